// wgsum.h -- a 256-thread workgroup's sums in a fixed order (the same bits on every call) and the
// kernel that folds partial sums with them; for the units whose kernels reduce this way.
#pragma once
#include "common.h"

// The tree: combine(t, h) folds entry t + h into entry t of LDS arrays that every thread has
// filled, for t < h, h = 128 .. 1; a barrier before the first level and after every level.
template <class F>
__device__ __forceinline__ void wg_tree(F combine)
{
    const int t = threadIdx.x;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h)
            combine(t, h);
        __syncthreads();
    }
}

// the sum of the 256 threads' v, in every thread; red: 256 doubles, free again on return
__device__ __forceinline__ double wg_tree_sum(double v, double (&red)[256])
{
    red[threadIdx.x] = v;
    wg_tree([&](int t, int h) { red[t] += red[t + h]; });
    const double r = red[0];
    __syncthreads();
    return r;
}

// two sums through one tree (one barrier per level for both), left in ra[0] and rb[0]
__device__ __forceinline__ void wg_tree_add2(double a, double b, double (&ra)[256], double (&rb)[256])
{
    ra[threadIdx.x] = a;
    rb[threadIdx.x] = b;
    wg_tree([&](int t, int h) { ra[t] += ra[t + h]; rb[t] += rb[t + h]; });
}

// NC sums per thread over four waves: the lanes by shuffles, then the waves through LDS in wave
// order.  Thread c < NC returns sum c.  red: 4 NC doubles, freed of their earlier use by a barrier
// here.  lane, wave: the caller's (a kernel may keep its wave index in a scalar register).
template <int NC>
__device__ __forceinline__ double wg_wave_sums(double (&sum)[NC], double *red, int lane, int wave)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int c = 0; c < NC; ++c)
            sum[c] += __shfl_xor(sum[c], off);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < NC; ++c)
            red[wave * NC + c] = sum[c];
    __syncthreads();
    return t < NC ? ((red[t] + red[NC + t]) + red[2 * NC + t]) + red[3 * NC + t] : 0.0;
}

// what fold_kernel multiplies sum c by: nothing, or the log-ML gradient's scalings
struct FoldPlain {};
__device__ __forceinline__ double fold_scaled(const FoldPlain &, int, double v) { return v; }
__device__ __forceinline__ double fold_scaled(const GradScale &s, int c, double v) { return v * s.f[c]; }

// out[c] = the sum over i < nitem of part[i item_stride + c c_stride], c < nc, scaled by sc: thread
// t adds items t, t + 256 .. in that order, then the tree.  Workgroup b takes c = b, b + gridDim.x
// ..; grid: any number of workgroups up to nc.
template <class Scale>
__global__ __launch_bounds__(256) void fold_kernel(const double *__restrict__ part, int nitem,
                                                   long item_stride, long c_stride, int nc,
                                                   Scale sc, double *__restrict__ out)
{
    __shared__ double red[256];
    for (int c = blockIdx.x; c < nc; c += gridDim.x) {
        double v = 0.0;
        for (int i = threadIdx.x; i < nitem; i += 256)
            v += part[i * item_stride + c * c_stride];
        v = wg_tree_sum(v, red);
        if (threadIdx.x == 0)
            out[c] = fold_scaled(sc, c, v);
    }
}
