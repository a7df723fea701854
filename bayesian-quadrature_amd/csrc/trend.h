// trend.h -- the polynomial trend of a resident fit, its coefficients marginalised (universal
// kriging with a flat prior; include/bqhip.h has the contract of bq_gp_trend and
// bq_gp_predict_trend).  Part of the libbqhip.so kernel set; compiled into k_reduce.hip.
//
// With H (n x p, rows phi(x_i)^T), G = L^-1 H, z = L^-1 y, A = G^T G, b = G^T z:
//   beta = A^-1 b,  alpha_t = L^-T (z - G beta),
//   r_j = phi(xo_j) - G^T v_j,  mean_t,j = v_j.z + r_j.beta,  var_t,j = k0 - |v_j|^2 + |L_A^-1 r_j|^2.
// G lives as the first p rows of a 64-row matrix (64 x npad, ld 64; its other rows and its columns
// at or beyond n are zero), as the solved vectors of ptheta.h do.
//   trend_basis_kernel   phi of d x m points into a zero-padded 64-row matrix (H; the query points)
//   trend_sums_kernel    a 64-column slice's share of A and b
//   trend_solve_kernel   one workgroup: L_A, beta, A^-1, log|A|, b^T beta, z - G beta, the status
//   rowdot_trend_kernel  rowdot_kernel's pass over V with the p <= 8 sums v.G_k riding along
//   trend_finish_kernel  mean += r.beta, var += |L_A^-1 r|^2
//   trend_mean_kernel    the route without a sweep: k(xo, x) alpha_t + phi(xo)^T beta
// No atomics and fixed orders throughout: the same bits on every call.
#pragma once
#include "common.h"

// phi's entries in the contract's order: 1; t_1 .. t_D; t_k t_l for k = 0 .. D - 1, l = k .. D - 1
template <int D, class F>
__device__ __forceinline__ void trend_phi(const double *x, const TrendBasis &tb, F emit)
{
    double t[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        t[k] = (x[k] - tb.c[k]) / tb.rho[k];
    emit(0, 1.0);
    if (tb.degree >= 1) {
#pragma unroll
        for (int k = 0; k < D; ++k)
            emit(1 + k, t[k]);
    }
    if (tb.degree >= 2) {
        int o = 1 + D;
#pragma unroll
        for (int k = 0; k < D; ++k)
#pragma unroll
            for (int l = k; l < D; ++l)
                emit(o++, t[k] * t[l]);
    }
}

// out[k rs + j cs] = phi_k(x_j) for j < m, zero for m <= j < mp and for every k in [p, 64).
// grid: ceil(mp / 256).
template <int D>
__global__ __launch_bounds__(256) void trend_basis_kernel(const double *__restrict__ x, int m,
                                                          int mp, TrendBasis tb,
                                                          double *__restrict__ out, long rs, long cs)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= mp)
        return;
    double *o = out + (long)j * cs;
    if (j < m) {
        double q[D];
#pragma unroll
        for (int k = 0; k < D; ++k)
            q[k] = x[k + (long)j * D];
        trend_phi<D>(q, tb, [&](int k, double v) { o[(long)k * rs] = v; });
        for (int k = tb.p; k < BQ_TREND_ROWS; ++k)
            o[(long)k * rs] = 0.0;
    } else {
        for (int k = 0; k < BQ_TREND_ROWS; ++k)
            o[(long)k * rs] = 0.0;
    }
}

// Workgroup b's share of A = G G^T and b = G z: the 64 columns [64 b, 64 b + 64) of G (64 x npad,
// ld 64), in column order, one fma per column.  part[b ne + e], ne = p p + p: e = k p + l is
// A[k, l] (both triangles: the same products in the same order, so A is symmetric to the bit),
// e = p p + k is b[k].  grid: npad / 64.
__global__ __launch_bounds__(256) void trend_sums_kernel(const double *__restrict__ G,
                                                         const double *__restrict__ z, int p,
                                                         double *__restrict__ part)
{
    __shared__ double Gs[64 * BQ_TREND_ROWS], zs[64];
    const int t = threadIdx.x;
    const double *g = G + (size_t)blockIdx.x * 64 * BQ_TREND_ROWS;
    for (int i = t; i < 64 * BQ_TREND_ROWS; i += 256)
        Gs[i] = g[i];
    if (t < 64)
        zs[t] = z[blockIdx.x * 64 + t];
    __syncthreads();
    const int ne = p * p + p;
    double *out = part + (size_t)blockIdx.x * ne;
    for (int e = t; e < ne; e += 256) {
        double s = 0.0;
        if (e < p * p) {
            const int k = e / p, l = e - k * p;
            for (int j = 0; j < 64; ++j)
                s = fma(Gs[k + BQ_TREND_ROWS * j], Gs[l + BQ_TREND_ROWS * j], s);
        } else {
            const int k = e - p * p;
            for (int j = 0; j < 64; ++j)
                s = fma(Gs[k + BQ_TREND_ROWS * j], zs[j], s);
        }
        out[e] = s;
    }
}

// One workgroup.  sums: A (p x p) | b (p).  The right-looking Cholesky of A in LDS; a pivot that
// is not positive and finite raises the status (the arithmetic runs on: nothing it feeds indexes
// memory, and the host hands out nothing).  Then, into tr (BQ_TREND_* offsets):
//   beta = L_A^-T (L_A^-1 b) (two substitutions), b^T beta = |L_A^-1 b|^2, log|A| = 2 sum log L_jj,
//   A^-1 = W^T W with W = L_A^-1 (a column of W per thread), L_A itself (ld p, zero above its
//   diagonal),
// and zt = z - G^T beta over the npad columns (one fma per basis row, in row order).
__global__ __launch_bounds__(256) void trend_solve_kernel(const double *__restrict__ sums, int p,
                                                          const double *__restrict__ G,
                                                          const double *__restrict__ z, int npad,
                                                          double *__restrict__ tr,
                                                          double *__restrict__ zt)
{
    constexpr int LD = BQ_TREND_MAXP + 1;
    __shared__ double La[BQ_TREND_MAXP * LD], W[BQ_TREND_MAXP * LD];
    __shared__ double bs[BQ_TREND_MAXP], ys[BQ_TREND_MAXP], be[BQ_TREND_ROWS];
    __shared__ int bad;
    const int t = threadIdx.x;
    for (int e = t; e < p * p; e += 256)
        La[(e / p) * LD + e % p] = sums[e];
    if (t < p)
        bs[t] = sums[p * p + t];
    if (t < BQ_TREND_ROWS)
        be[t] = 0.0;
    if (t == 0)
        bad = 0;
    __syncthreads();
    for (int j = 0; j < p; ++j) {
        if (t == 0) {
            const double dj = La[j * LD + j];
            if (!(dj > 0.0) || !(dj <= 1.7976931348623157e308))
                bad = 1;
            La[j * LD + j] = sqrt(dj);
        }
        __syncthreads();
        const double piv = La[j * LD + j];
        if (t > j && t < p)
            La[t * LD + j] /= piv;
        __syncthreads();
        // rows i > j, columns j < l <= i
        const int m = p - j - 1;
        for (int e = t; e < m * m; e += 256) {
            const int i = j + 1 + e / m, l = j + 1 + e % m;
            if (l <= i)
                La[i * LD + l] = fma(-La[i * LD + j], La[l * LD + j], La[i * LD + l]);
        }
        __syncthreads();
    }
    // W = L_A^-1, column t by forward substitution
    if (t < p) {
        for (int i = 0; i < p; ++i) {
            double s = i == t ? 1.0 : 0.0;
            for (int k = t; k < i; ++k)
                s = fma(-La[i * LD + k], W[k * LD + t], s);
            W[i * LD + t] = i < t ? 0.0 : s / La[i * LD + i];
        }
    }
    if (t == 64) { // another wave: y = L_A^-1 b, beta = L_A^-T y, the scalars
        double q = 0.0, lg = 0.0;
        for (int i = 0; i < p; ++i) {
            double s = bs[i];
            for (int k = 0; k < i; ++k)
                s = fma(-La[i * LD + k], ys[k], s);
            s /= La[i * LD + i];
            ys[i] = s;
            q = fma(s, s, q);
            lg += log(La[i * LD + i]);
        }
        for (int i = p - 1; i >= 0; --i) {
            double s = ys[i];
            for (int k = i + 1; k < p; ++k)
                s = fma(-La[k * LD + i], be[k], s);
            be[i] = s / La[i * LD + i];
        }
        tr[BQ_TREND_STATUS] = bad ? 1.0 : 0.0;
        tr[BQ_TREND_LOGDET] = 2.0 * lg;
        tr[BQ_TREND_BTB] = q;
    }
    __syncthreads();
    if (t < BQ_TREND_ROWS)
        tr[BQ_TREND_BETA + t] = be[t];
    for (int e = t; e < p * p; e += 256) {
        const int k = e % p, l = e / p; // entry (k, l) at k + l p
        double s = 0.0;
        for (int i = (k > l ? k : l); i < p; ++i)
            s = fma(W[i * LD + k], W[i * LD + l], s);
        tr[BQ_TREND_AINV + e] = s;
        tr[BQ_TREND_LA + e] = k >= l ? La[k * LD + l] : 0.0;
    }
    for (int j = t; j < npad; j += 256) {
        const double *g = G + (size_t)j * BQ_TREND_ROWS;
        double s = z[j];
        for (int k = 0; k < p; ++k)
            s = fma(-g[k], be[k], s);
        zt[j] = s;
    }
}

// rowdot_kernel (reduce.h) with NB sums more: mean_i = v_i.z and var_i = k0 - |v_i|^2 are its bits
// -- the same loads in flight, the same chains of fma in the same order -- and row i of R
// (m x 64, ld ldr; on entry phi(xo_i)) leaves as r_i = phi(xo_i) - G^T v_i in its first NB entries.
// The slice's G entries (G: 64 x n, ld 64; NB contiguous doubles per column) are one address for
// the 16 rows of a slice.  block = 16 rows x 64 column slices; grid: ceil(m / 16).
template <int NB>
__global__ __launch_bounds__(1024) void rowdot_trend_kernel(const double *__restrict__ V, long ldv,
                                                            int m, int n,
                                                            const double *__restrict__ z, double k0,
                                                            const double *__restrict__ G,
                                                            double *__restrict__ mean,
                                                            double *__restrict__ var,
                                                            double *__restrict__ R, long ldr)
{
    const int t = threadIdx.x, r = t & 15, sl = t >> 4;
    const int row = blockIdx.x * 16 + r;
    double sm = 0.0, sv = 0.0, sg[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k)
        sg[k] = 0.0;
    if (row < m) {
        const double *p = V + row;
        int j = sl;
        for (; j + 64 * 15 < n; j += 64 * 16) {
            double v[16], zz[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                v[u] = p[(long)(j + 64 * u) * ldv];
                zz[u] = z[j + 64 * u];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                sm = fma(v[u], zz[u], sm);
                sv = fma(v[u], v[u], sv);
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const double *g = G + (size_t)(j + 64 * u) * BQ_TREND_ROWS;
#pragma unroll
                for (int k = 0; k < NB; ++k)
                    sg[k] = fma(v[u], g[k], sg[k]);
            }
        }
        for (; j + 64 * 7 < n; j += 64 * 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                v[u] = p[(long)(j + 64 * u) * ldv];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                sm = fma(v[u], z[j + 64 * u], sm);
                sv = fma(v[u], v[u], sv);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double *g = G + (size_t)(j + 64 * u) * BQ_TREND_ROWS;
#pragma unroll
                for (int k = 0; k < NB; ++k)
                    sg[k] = fma(v[u], g[k], sg[k]);
            }
        }
        for (; j < n; j += 64) {
            const double v = p[(long)j * ldv];
            sm = fma(v, z[j], sm);
            sv = fma(v, v, sv);
            const double *g = G + (size_t)j * BQ_TREND_ROWS;
#pragma unroll
            for (int k = 0; k < NB; ++k)
                sg[k] = fma(v, g[k], sg[k]);
        }
    }
    __shared__ double pm[64][17], pv[64][17];
    pm[sl][r] = sm;
    pv[sl][r] = sv;
    __syncthreads();
    if (t < 16 && row < m) {
        double a = 0.0, q = 0.0;
        for (int w = 0; w < 64; ++w) {
            a += pm[w][r];
            q += pv[w][r];
        }
        mean[row] = a;
        var[row] = k0 - q;
    }
    // the NB sums through the same two arrays, two at a time, in slice order like the others
#pragma unroll
    for (int k = 0; k < NB; k += 2) {
        __syncthreads();
        pm[sl][r] = sg[k];
        if (k + 1 < NB)
            pv[sl][r] = sg[k + 1];
        __syncthreads();
        if (t < 16 && row < m) {
            double a = 0.0, q = 0.0;
            for (int w = 0; w < 64; ++w) {
                a += pm[w][r];
                if (k + 1 < NB)
                    q += pv[w][r];
            }
            R[row + (long)k * ldr] -= a;
            if (k + 1 < NB)
                R[row + (long)(k + 1) * ldr] -= q;
        }
    }
}

// mean_j += r_j.beta, var_j += |L_A^-1 r_j|^2 for j < m: one point per thread, L_A (ld p) and beta
// in LDS, the substitution's u in LDS too (entry k of the 64 threads side by side).  R: m x 64, ld
// ldr.  status[0] = the solve's status, for the one read-back.  block: 64; grid: ceil(m / 64).
__global__ __launch_bounds__(64) void trend_finish_kernel(const double *__restrict__ R, long ldr,
                                                          int m, int p,
                                                          const double *__restrict__ tr,
                                                          double *__restrict__ mean,
                                                          double *__restrict__ var,
                                                          double *__restrict__ status)
{
    __shared__ double La[BQ_TREND_MAXP * BQ_TREND_MAXP], be[BQ_TREND_MAXP];
    __shared__ double us[BQ_TREND_MAXP][64];
    const int t = threadIdx.x, j = blockIdx.x * 64 + t;
    for (int e = t; e < p * p; e += 64)
        La[e] = tr[BQ_TREND_LA + e];
    if (t < p)
        be[t] = tr[BQ_TREND_BETA + t];
    if (blockIdx.x == 0 && t == 0)
        status[0] = tr[BQ_TREND_STATUS];
    __syncthreads();
    if (j >= m)
        return;
    double dm = 0.0, dv = 0.0;
    for (int i = 0; i < p; ++i) {
        const double ri = R[j + (long)i * ldr];
        dm = fma(ri, be[i], dm);
        double s = ri;
        for (int k = 0; k < i; ++k)
            s = fma(-La[i + k * p], us[k][t], s);
        s /= La[i + i * p];
        us[i][t] = s;
        dv = fma(s, s, dv);
    }
    mean[j] += dm;
    var[j] += dv;
}

// mean_i = sum_j k(xo_i, x_j) alpha_t,j + phi(xo_i)^T beta: predict_mean_kernel's pattern (one wave
// per point, the lanes stride over j), the trend's term added by lane 0.  status as above.
template <int D>
__global__ __launch_bounds__(256) void trend_mean_kernel(const double *__restrict__ xo, int M,
                                                         const double *__restrict__ x, int n,
                                                         const double *__restrict__ alpha,
                                                         GaussParams g, TrendBasis tb,
                                                         const double *__restrict__ tr,
                                                         double *__restrict__ mean,
                                                         double *__restrict__ status)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        status[0] = tr[BQ_TREND_STATUS];
    if (i >= M)
        return;
    double p[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        p[k] = xo[k + (long)i * D];
    double s = 0.0;
    for (int j = lane; j < n; j += 64) {
        double q[D];
#pragma unroll
        for (int k = 0; k < D; ++k)
            q[k] = x[k + (long)j * D];
        s += exp_gauss(gauss_q<D>(p, q, g)) * alpha[j];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        s += __shfl_down(s, off, 64);
    if (lane == 0) {
        double b = 0.0;
        const double *be = tr + BQ_TREND_BETA;
        trend_phi<D>(p, tb, [&](int k, double v) { b = fma(v, be[k], b); });
        mean[i] = g.c * s + b;
    }
}
