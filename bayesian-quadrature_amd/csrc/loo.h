// loo.h -- leave-one-out cross-validation of a resident fit (bq_gp_loo, bq_gp_loo_grad, fit.hip).
//
// With Ki = Kxx^-1 = Y Y^T (Y = L^-T), a = Ki y and k_i = Ki_ii (Rasmussen & Williams 5.4.2):
//   mu_i = y_i - a_i / k_i,  var_i = 1 / k_i,  lp_i = 1/2 log k_i - a_i^2 / (2 k_i) - 1/2 log 2 pi
//   L_loo = sum_i lp_i
//   dL_loo / dtheta_p = sum_i [a_i (Z_p a)_i - 1/2 (1 + a_i^2 / k_i) (Z_p Ki)_ii] / k_i,  Z_p = Ki D_p
// (Z_p a) is the Hessian's resident vector Ki (D_p a) (hess.h), and with q_i = sum_m Ki_im^2 and
// t_ki = sum_m B_k(i, m) Ki(m, i), B_k = Ki D_k:
//   (Z_h Ki)_ii = (2 / h)(k_i - s^2 q_i),  (Z_k Ki)_ii = t_ki,  (Z_s Ki)_ii = 2 s q_i
// Nothing cubic: every kernel here reads each matrix entry once.
//
//   loo_diag_kernel     k_i = sum_{m >= i} Y(i, m)^2, partial over a chunk of columns
//   loo_rows_kernel<D>  q_i and t_1i .. t_di, partial over a chunk of columns (Ki(m, i) read as
//                       Ki(i, m): Ki is stored in full and symmetric)
//   loo_fold_kernel     a row's partials over the chunks, in their order
//   loo_point_kernel    mu, var, lp and their sum L_loo
//   loo_grad_kernel<D>  the d + 2 gradient entries
// All matrices are column-major with ld npad: lanes go along rows, so a wave's load of one column
// is 64 consecutive doubles.  A workgroup owns 64 rows and BQ_LOO_CW columns, its four waves take
// every fourth column; rows and columns at or beyond n (the identity padding) stay out of every
// sum.  No atomics: the same bits on every call (the workgroup-wide sums are wgsum.h's tree).
#pragma once
#include "common.h"
#include "wgsum.h"

#define BQ_LOO_CW 256 // columns per workgroup

constexpr double BQ_HALF_LOG_2PI = 0.91893853320467274178;

// The four waves' sums of one row each, wave 0 .. 3 in that order.
// part: [NC][nchunk][npad]; red: 3 * NC * 64 doubles
template <int NC>
__device__ __forceinline__ void loo_row_sums(const double (&sum)[NC], double *red,
                                             double *__restrict__ part, int chunk, int nchunk,
                                             int npad, int i)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave)
#pragma unroll
        for (int c = 0; c < NC; ++c)
            red[((wave - 1) * NC + c) * 64 + lane] = sum[c];
    __syncthreads();
    if (wave == 0)
#pragma unroll
        for (int c = 0; c < NC; ++c)
            part[((long)c * nchunk + chunk) * npad + i] =
                ((sum[c] + red[c * 64 + lane]) + red[(NC + c) * 64 + lane]) +
                red[(2 * NC + c) * 64 + lane];
}

// grid: (npad / 64, nchunk); part: [1][nchunk][npad]
__global__ __launch_bounds__(256) void loo_diag_kernel(const double *__restrict__ Y, int n, int npad,
                                                       double *__restrict__ part)
{
    __shared__ double red[3 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R0 = blockIdx.x * 64, i = R0 + lane;
    const int c0 = blockIdx.y * BQ_LOO_CW, cend = min(c0 + BQ_LOO_CW, n);
    double sum[1] = {0.0};
    if (i < n) {
        // (Y is upper triangular: the columns left of this row block hold nothing)
#pragma unroll 8
        for (int m = max(c0, R0) + wave; m < cend; m += 4)
            if (m >= i) {
                const double v = Y[i + (long)m * npad];
                sum[0] += v * v;
            }
    }
    loo_row_sums<1>(sum, red, part, blockIdx.y, gridDim.y, npad, i);
}

// B: the d products B_k = Ki D_k, npad^2 apart.  grid: (npad / 64, nchunk);
// part: [1 + D][nchunk][npad] -- q, t_1 .. t_D
template <int D>
__global__ __launch_bounds__(256) void loo_rows_kernel(const double *__restrict__ Ki,
                                                       const double *__restrict__ B, int n,
                                                       int npad, double *__restrict__ part)
{
    constexpr int NC = 1 + D;
    __shared__ double red[3 * NC * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const int c0 = blockIdx.y * BQ_LOO_CW, cend = min(c0 + BQ_LOO_CW, n);
    const long bs = (long)npad * npad;
    double sum[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
        sum[c] = 0.0;
    if (i < n) {
#pragma unroll 4
        for (int m = c0 + wave; m < cend; m += 4) {
            const long o = i + (long)m * npad;
            const double kv = Ki[o];
            sum[0] += kv * kv;
#pragma unroll
            for (int k = 0; k < D; ++k)
                sum[1 + k] += B[k * bs + o] * kv;
        }
    }
    loo_row_sums<NC>(sum, red, part, blockIdx.y, gridDim.y, npad, i);
}

// out[c][i] = part[c][0 .. nchunk)[i] summed in that order.  grid: (npad / 256, the sums)
__global__ __launch_bounds__(256) void loo_fold_kernel(const double *__restrict__ part, int nchunk,
                                                       int npad, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (i >= npad)
        return;
    double v = 0.0;
    for (int ch = 0; ch < nchunk; ++ch)
        v += part[((long)c * nchunk + ch) * npad + i];
    out[(long)c * npad + i] = v;
}

// mu, var, lp for i < n and *total = L_loo.  One workgroup.
__global__ __launch_bounds__(256) void loo_point_kernel(const double *__restrict__ y,
                                                        const double *__restrict__ a,
                                                        const double *__restrict__ kd, int n,
                                                        double *__restrict__ mu,
                                                        double *__restrict__ var,
                                                        double *__restrict__ lp,
                                                        double *__restrict__ total)
{
    __shared__ double red[256];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double ki = kd[i], ai = a[i];
        const double r = ai / ki;
        const double l = 0.5 * log(ki) - 0.5 * (ai * r) - BQ_HALF_LOG_2PI;
        mu[i] = y[i] - r;
        var[i] = 1.0 / ki;
        lp[i] = l;
        v += l;
    }
    v = wg_tree_sum(v, red);
    if (threadIdx.x == 0)
        *total = v;
}

// out[p] = dL_loo / dtheta_p over [h, w_1 .. w_D, s].  tk: t_1 .. t_D and Z: the D + 2 vectors
// Ki (D_p a), both npad apart.  One workgroup.
template <int D>
__global__ __launch_bounds__(256) void loo_grad_kernel(const double *__restrict__ a,
                                                       const double *__restrict__ kd,
                                                       const double *__restrict__ q,
                                                       const double *__restrict__ tk,
                                                       const double *__restrict__ Z, int n,
                                                       int npad, double two_over_h, double s,
                                                       double s2, double *__restrict__ out)
{
    __shared__ double red[256];
#pragma unroll
    for (int p = 0; p < D + 2; ++p) {
        double v = 0.0;
        for (int i = threadIdx.x; i < n; i += 256) {
            const double ki = kd[i], ai = a[i];
            double dg; // (Z_p Ki)_ii
            if (p == 0)
                dg = two_over_h * (ki - s2 * q[i]);
            else if (p == D + 1)
                dg = 2.0 * s * q[i];
            else
                dg = tk[(long)(p - 1) * npad + i];
            v += (ai * Z[(long)p * npad + i] - 0.5 * (1.0 + ai * ai / ki) * dg) / ki;
        }
        v = wg_tree_sum(v, red);
        if (threadIdx.x == 0)
            out[p] = v;
    }
}
