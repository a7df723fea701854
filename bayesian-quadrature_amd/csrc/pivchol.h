// pivchol.h -- the greedy, diagonally pivoted partial Cholesky factorisation of a resident fit's
// posterior covariance Sigma = K(xo, xo) - V V^T, which is never formed (fit.hip, bq_gp_pivchol;
// include/bqhip.h has the contract).
// Part of the libbqhip.so kernel set; compiled into k_reduce.hip (host.h lists the units).
//
// The factor's columns follow V in one matrix W = [V | C] (Mp x (npad + q), ld Mp).  Step j with
// pivot p:
//     c_j = (K(xo, xo_p) - W[:, :npad + j] W[p, :npad + j]^T) / sqrt(gain_j + nugget),
//     d  -= c_j o c_j,
// and the next pivot is the first largest entry of d.  Three launches a step, none of which
// waits for the host: the pivot, its gain and the done flag live in a PivcholState on the device.
//   pivchol_col_kernel     the row-gathered product, cut along k into slices of KS columns:
//                          part[slice][row]
//   pivchol_finish_kernel  the slices summed in order, the kernel value, the division, column
//                          npad + j of W, d, and each workgroup's (max, argmax) of the new d
//   pivchol_select_kernel  one workgroup: the argmax over the workgroups' candidates, the stop
//                          rule, piv[j + 1], gain[j + 1], the done flag
// After the done flag every kernel returns at once.
//
// Determinism: KS comes from (Mp, npad) alone (k_reduce.hip, pivchol_plan), a slice's sum is
// BQ_PIVCHOL_U accumulators that take their k steps in ascending order and are folded in a fixed
// tree, and the slices are added in ascending order: a column's bits depend on (Mp, npad, j) and
// never on q, so the first j columns of a q-step call are those of a j-step call, and two calls
// give the same bits.  No floating-point atomics.
#pragma once
#include "common.h"
#include <limits.h>

constexpr int BQ_PIVCHOL_KS_MAX = 512; // columns per slice at most: the piece of W[p, :] in LDS
constexpr int BQ_PIVCHOL_U = 16;       // a thread's independent accumulators = its loads in flight

// whether candidate (v, i) comes before (bv, bi): the larger value, the lower index among equals;
// a NaN comes before every number, so that a poisoned diagonal stops the factorisation
__device__ __forceinline__ bool pivchol_before(double v, int i, double bv, int bi)
{
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn)
        return vn;
    return (!vn && v > bv) || ((vn || v == bv) && i < bi);
}

// the first of a 256-thread workgroup's candidates, left in sv[0], si[0]
__device__ __forceinline__ void pivchol_wg_first(double v, int i, double *sv, int *si)
{
    const int t = threadIdx.x;
    sv[t] = v, si[t] = i;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h && pivchol_before(sv[t + h], si[t + h], sv[t], si[t]))
            sv[t] = sv[t + h], si[t] = si[t + h];
        __syncthreads();
    }
}

// d = var on the M real rows (bq_gp_predict's latent variance: d^(0) = diag Sigma), 0 on the
// padding; no row taken; each workgroup's candidate; workgroup 0: piv = -1, gain = 0, the state
// with rank = q.  grid ceil(Mp / 256).
__global__ __launch_bounds__(256) void pivchol_init_kernel(const double *__restrict__ var, int M,
                                                           int Mp, int q, PivcholState *st,
                                                           long long *__restrict__ piv,
                                                           double *__restrict__ gain,
                                                           double *__restrict__ d,
                                                           int *__restrict__ taken,
                                                           double *__restrict__ candv,
                                                           int *__restrict__ candi)
{
    __shared__ double sv[256];
    __shared__ int si[256];
    const int t = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + t;
    double v = -INFINITY;
    int idx = INT_MAX;
    if (i < Mp) {
        const double di = i < M ? var[i] : 0.0;
        d[i] = di;
        taken[i] = 0;
        if (i < M)
            v = di, idx = (int)i;
    }
    if (blockIdx.x == 0) {
        for (int k = t; k < q; k += 256)
            piv[k] = -1, gain[k] = 0.0;
        if (t == 0)
            st->done = 0, st->rank = q, st->p = 0, st->pad = 0, st->gain = 0.0;
    }
    pivchol_wg_first(v, idx, sv, si);
    if (t == 0)
        candv[blockIdx.x] = sv[0], candi[blockIdx.x] = si[0];
}

// Step j's pivot out of the nblk candidates, or the end: rank = j and the done flag when the gain
// is at most thr (= tol k0), not positive or not finite.  One workgroup of 256 threads.
__global__ __launch_bounds__(256) void pivchol_select_kernel(PivcholState *st,
                                                             const double *__restrict__ candv,
                                                             const int *__restrict__ candi,
                                                             int nblk, int j, double thr,
                                                             long long *__restrict__ piv,
                                                             double *__restrict__ gain)
{
    __shared__ double sv[256];
    __shared__ int si[256];
    if (st->done)
        return;
    const int t = threadIdx.x;
    double v = -INFINITY;
    int idx = INT_MAX;
    for (int b = t; b < nblk; b += 256) {
        const double bv = candv[b];
        const int bi = candi[b];
        if (pivchol_before(bv, bi, v, idx))
            v = bv, idx = bi;
    }
    pivchol_wg_first(v, idx, sv, si);
    if (t == 0) {
        const double g = sv[0];
        if (g > thr && g > 0.0 && g < INFINITY) {
            st->p = si[0], st->gain = g;
            piv[j] = si[0], gain[j] = g;
        } else {
            st->done = 1, st->rank = j;
        }
    }
}

// part[slice y][row] = sum over k in the slice of W[row, k] W[p, k], K = npad + j columns in
// slices of KS <= BQ_PIVCHOL_KS_MAX.  grid (Mp / RB, ceil(K / KS)), RB threads, one row each: a
// load of W[:, k] is coalesced.  The slice's piece of W[p, :] is gathered by the workgroup itself
// (stride ld, one value per k) into LDS.  BQ_PIVCHOL_U loads leave before the first use.
template <int RB>
__global__ __launch_bounds__(RB) void pivchol_col_kernel(const double *__restrict__ W, long ld,
                                                         int K, int KS, const PivcholState *st,
                                                         double *__restrict__ part)
{
    constexpr int U = BQ_PIVCHOL_U;
    __shared__ double u[BQ_PIVCHOL_KS_MAX];
    if (st->done)
        return;
    const int t = threadIdx.x, p = st->p;
    const long row = (long)blockIdx.x * RB + t;
    const int k0 = (int)blockIdx.y * KS, len = min(KS, K - k0);
    for (int k = t; k < len; k += RB)
        u[k] = W[p + (long)(k0 + k) * ld];
    __syncthreads();
    const double *w = W + row + (long)k0 * ld;
    double acc[U];
#pragma unroll
    for (int i = 0; i < U; ++i)
        acc[i] = 0.0;
    int k = 0;
    for (; k + U <= len; k += U) {
        double a[U];
#pragma unroll
        for (int i = 0; i < U; ++i)
            a[i] = w[(long)(k + i) * ld];
#pragma unroll
        for (int i = 0; i < U; ++i)
            acc[i] = __builtin_fma(a[i], u[k + i], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < U; ++i)
        if (k + i < len)
            acc[i] = __builtin_fma(w[(long)(k + i) * ld], u[k + i], acc[i]);
#pragma unroll
    for (int h = U / 2; h >= 1; h >>= 1)
#pragma unroll
        for (int i = 0; i < h; ++i)
            acc[i] += acc[i + h];
    part[(long)blockIdx.y * ld + row] = acc[0];
}

// Column npad + j of W and the new d, row by row; grid ceil(Mp / 256).  Real rows: the nsl slices
// in order, k(xo_row, xo_p) with gram_cross_kernel's arithmetic (g: the fit's parameters, its s^2
// not used), the division by sqrt(gain + nugget).  nugget = 0: the pivot's own entry is
// sqrt(gain) and its d an exact 0, and a row taken earlier stores an exact 0 and keeps d = 0.
// Padding rows store 0 and are no candidates.
template <int D>
__global__ __launch_bounds__(256) void pivchol_finish_kernel(
    double *__restrict__ W, long ld, int col, int M, int Mp, const double *__restrict__ part,
    int nsl, const double *__restrict__ xq, GaussParams g, double nugget,
    const PivcholState *st, double *__restrict__ d, int *__restrict__ taken,
    double *__restrict__ candv, int *__restrict__ candi)
{
    __shared__ double sv[256];
    __shared__ int si[256];
    if (st->done)
        return;
    const int t = threadIdx.x, p = st->p;
    const double den = sqrt(st->gain + nugget);
    const long i = (long)blockIdx.x * 256 + t;
    double v = -INFINITY;
    int idx = INT_MAX;
    if (i < Mp) {
        double cv = 0.0;
        if (i < M) {
            double s = 0.0;
            for (int y = 0; y < nsl; ++y)
                s += part[(long)y * ld + i];
            const double kv = g.c * exp_gauss(gauss_q<D>(xq + i * D, xq + (long)p * D, g));
            double di = d[i];
            if (nugget == 0.0 && i == p) {
                cv = den, di = 0.0;
                taken[i] = 1;
            } else if (nugget == 0.0 && taken[i]) {
                di = 0.0;
            } else {
                cv = (kv - s) / den;
                di = __builtin_fma(-cv, cv, di);
            }
            d[i] = di;
            v = di, idx = (int)i;
        }
        W[i + (long)col * ld] = cv;
    }
    pivchol_wg_first(v, idx, sv, si);
    if (t == 0)
        candv[blockIdx.x] = sv[0], candi[blockIdx.x] = si[0];
}
