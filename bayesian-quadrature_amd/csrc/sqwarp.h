// sqwarp.h -- square-root-warped Bayesian quadrature of a resident fit (WSABI-L, Gunter et al.
// 2014): the pair sums of its kernel means (fit.hip, bq_gp_sqintegral and bq_gp_sqdesign;
// include/bqhip.h has the contracts).
// Part of the libbqhip.so kernel set; compiled into k_reduce.hip (host.h lists the units).
//
// The fit's targets are g = sqrt(2 (l - alpha0)); l = alpha0 + g^2 / 2 linearised about the
// posterior mean m = k(., X) alpha is a GP again, and Z = int m g pi has kernel means that are sums
// over pairs of points:
//     out[a] = sum_j W(p_a, x_j) alpha_j,   W(p, q) = int k(p, t) k(t, q) pi(t) dt
//            = h^4 N(p - q | 0, 2 Lambda) N((p + q) / 2 | mu, Lambda / 2 + Sigma).
// Every point is transformed once (sq_xform_kernel) to 2d coordinates
//     t1 = p / (sqrt 2 w),   t2 = Linv (p - mu) / 2,   Linv^T Linv = (Lambda / 2 + Sigma)^-1,
// after which a pair costs 4d subtract / FMA and one exp (sq_pair_kernel):
//     W(p, q) = cw exp(-|t1(p) - t1(q)|^2 / 2 - |t2(p) + t2(q)|^2 / 2).
// Differences and sums of coordinates, never the expanded bilinear form, whose cancellation grows
// with |t|^2.  The prior variance's bilinear form alpha^T Q alpha (Q = int int k K k, moments.h's
// int_int_K1_K2_K1 with K1 = K2) is the same sum over d difference coordinates and no sums, with
// the points' own Gaussian factors in the weights.
//   sq_xform_kernel   the coordinates of n points and their weights, zero on the padding
//   sq_pair_kernel    part[slice][row] = sum over the slice's columns, one thread per row
//   sq_fold_kernel    the slices added in ascending order, times the constant in front
//
// Determinism: a row's sum over a slice is taken by one thread, column j of the slice into
// accumulator j mod 4, the four folded in a fixed tree; the slices' widths depend on the shapes
// alone (sq_pair_plan).  No floating-point atomics.
#pragma once
#include "zdesign.h"

// t[i] = [a1 x_i | a2 (x_i - m2)] (the second half with NS = D only), ND + NS doubles per point;
// wt[i] = alpha[i] (1 without alpha), with NS = 0 times exp(klogc - |kl (x_i - km)|^2 / 2).  Points
// n .. np - 1 get zero coordinates and weight 0.  wt may be NULL.  grid ceil(np / 256).
template <int D, int NS>
__global__ __launch_bounds__(256) void sq_xform_kernel(const double *__restrict__ x, int n, int np,
                                                       SqXform<D> f,
                                                       const double *__restrict__ alpha,
                                                       double *__restrict__ t,
                                                       double *__restrict__ wt)
{
    constexpr int NC = D + NS;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= np)
        return;
    double c[NC], wv = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k)
        c[k] = 0.0;
    if (i < n) {
        double xi[D];
#pragma unroll
        for (int k = 0; k < D; ++k)
            xi[k] = x[k + (long)i * D];
#pragma unroll
        for (int r = 0; r < D; ++r) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k)
                s = __builtin_fma(f.a1[r * D + k], xi[k], s);
            c[r] = s;
        }
        if (NS) {
#pragma unroll
            for (int r = 0; r < NS; ++r) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k)
                    s = __builtin_fma(f.a2[r * D + k], xi[k] - f.m2[k], s);
                c[D + r] = s;
            }
        }
        wv = alpha ? alpha[i] : 1.0;
        if (!NS) {
            double maha = 0.0;
#pragma unroll
            for (int r = 0; r < D; ++r) {
                double y = 0.0;
#pragma unroll
                for (int k = 0; k <= r; ++k)
                    y = __builtin_fma(f.kl[r * D + k], xi[k] - f.km[k], y);
                maha = __builtin_fma(y, y, maha);
            }
            wv *= exp(f.klogc - 0.5 * maha);
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k)
        t[(long)i * NC + k] = c[k];
    if (wt)
        wt[i] = wv;
}

// part[slice y][row] = sum over the columns j of slice y of
//     exp(-sum_{k < ND} (tp[row][k] - tx[j][k])^2 / 2
//         -sum_{ND <= k < NC} (tp[row][k] + tx[j][k])^2 / 2) wt[j]
// for the R row points tp (NC = ND + NS doubles each) against the n column points tx with their
// weights; slice y holds the columns [y JS, min((y + 1) JS, n)), JS a multiple of BQ_SQ_TJ.
// grid (ceil(ldp / 256), slices), 256 threads, one row each with its coordinates in registers; the
// columns go through LDS BQ_SQ_TJ at a time and are read by broadcast (every lane the same
// address).  Rows R .. ldp - 1 store an exact 0; columns from n on are never read.
template <int ND, int NS>
__global__ __launch_bounds__(BQ_SQ_RB) void sq_pair_kernel(const double *__restrict__ tp, int R,
                                                           long ldp, const double *__restrict__ tx,
                                                           const double *__restrict__ wt, int n,
                                                           int JS, double *__restrict__ part)
{
    constexpr int NC = ND + NS, TJ = BQ_SQ_TJ;
    __shared__ double sx[TJ * NC];
    __shared__ double sw[TJ];
    const int t = threadIdx.x;
    const long row = (long)blockIdx.x * BQ_SQ_RB + t;
    double p[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k)
        p[k] = row < R ? tp[row * NC + k] : 0.0;
    const int j0 = (int)blockIdx.y * JS, j1 = min(j0 + JS, n);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    auto term = [&](int j) {
        const double *xj = sx + j * NC;
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const double e = p[k] - xj[k];
            q = __builtin_fma(e, e, q);
        }
#pragma unroll
        for (int k = ND; k < NC; ++k) {
            const double e = p[k] + xj[k];
            q = __builtin_fma(e, e, q);
        }
        return exp_gauss(-0.5 * q);
    };
    for (int jt = j0; jt < j1; jt += TJ) {
        const int len = min(TJ, j1 - jt);
        __syncthreads(); // the tile before this one has been read
        for (int k = t; k < len * NC; k += BQ_SQ_RB)
            sx[k] = tx[(long)jt * NC + k];
        for (int k = t; k < len; k += BQ_SQ_RB)
            sw[k] = wt[jt + k];
        __syncthreads();
        int j = 0;
        for (; j + 4 <= len; j += 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i] = __builtin_fma(term(j + i), sw[j + i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (j + i < len)
                acc[i] = __builtin_fma(term(j + i), sw[j + i], acc[i]);
    }
    if (row < ldp)
        part[(long)blockIdx.y * ldp + row] = row < R ? (acc[0] + acc[1]) + (acc[2] + acc[3]) : 0.0;
}

// out[i] = scale (part[0][i] + part[1][i] + ..), the nsl slices ld apart, in ascending order, for
// the R rows; an exact 0 on rows R .. Rp - 1.  grid ceil(Rp / 256).
__global__ __launch_bounds__(256) void sq_fold_kernel(const double *__restrict__ part, long ld,
                                                      int nsl, int R, int Rp, double scale,
                                                      double *__restrict__ out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Rp)
        return;
    double s = 0.0;
    if (i < R) {
        for (int y = 0; y < nsl; ++y)
            s += part[(long)y * ld + i];
        s *= scale;
    }
    out[i] = s;
}
