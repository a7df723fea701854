// pgrad.h -- gradients of the posterior mean and variance with respect to the query points
// Part of the libbqhip.so kernel set; compiled into k_reduce.hip (host.h lists the units).
//
//   k_ji = k(xo_j, x_i),   e_jik = (x_ik - xo_jk) / w_k^2 = -2 nh[k] (x_ik - xo_jk)
//   d mean_j / d xo_jk =      sum_i k_ji e_jik alpha_i        alpha  = Kxx^-1 y
//   d var_j  / d xo_jk = -2   sum_i k_ji e_jik beta_ji        beta_j = Kxx^-1 k_j
//
// Determinism as in reduce.h and loo.h: every sum has a fixed order (a thread's columns in
// sequence, a shuffle tree, then partials in index order) and there are no atomics, so two calls
// give the same bits.  The kernels sum k_ji (x_ik - xo_jk) alpha_i without the constants; c,
// -2 nh[k] and the variance's -2 are applied once to the finished sums.
#pragma once
#include "common.h"

// Both gradients from beta (Mp x npad, ld = ldb, rows along the fast index: what the backward row
// sweep of bq_gp_predict_grad leaves) and alpha.  The decomposition of rowdot_kernel: a block is
// 16 rows x 64 column slices (1024 threads; a wave reads four columns of beta x 128 bytes and, for
// each, one point and one alpha that its 16 row lanes share), a thread keeps its query point in
// registers and recomputes k_ji, since the cross Gram is gone by now.  Only i < n and row < m are
// ever read or summed: the padding rows and columns of beta and the padding points do not enter.
// beta == nullptr: no dvar; alpha == nullptr: no dmean.  xo may be mapped host memory (each
// workgroup reads its 16 points once).  dmean, dvar: d x m, entry [k + row d].  grid: ceil(m / 16).
// LDS: 16 waves x 2 D x 16 rows of partial sums (32 KB at D = 8) -- the four slices of a row that
// share a wave are folded by shuffles first.
template <int D>
__global__ __launch_bounds__(1024) void predict_grad_kernel(const double *__restrict__ beta,
                                                            long ldb, int m,
                                                            const double *__restrict__ xo,
                                                            const double *__restrict__ x, int n,
                                                            const double *__restrict__ alpha,
                                                            GaussParams g,
                                                            double *__restrict__ dmean,
                                                            double *__restrict__ dvar)
{
    const int t = threadIdx.x, r = t & 15, sl = t >> 4, wave = t >> 6;
    const int row = blockIdx.x * 16 + r;
    const bool live = row < m;
    double p[D], sv[D], sm[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        p[k] = live ? xo[k + (long)row * D] : 0.0;
        sv[k] = 0.0;
        sm[k] = 0.0;
    }
    if (live) {
        const double *bp = beta ? beta + row : nullptr;
        int i = sl;
        // (U columns per trip: their loads leave together, the exponentials follow; two from
        // D = 5 on, where four sets of coordinates no longer fit the 128 registers of a
        // 1024-thread block)
        constexpr int U = D <= 4 ? 4 : 2;
        for (; i + 64 * (U - 1) < n; i += 64 * U) {
            double q[U][D], b[U], a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int iu = i + 64 * u;
#pragma unroll
                for (int k = 0; k < D; ++k)
                    q[u][k] = x[k + (long)iu * D];
                b[u] = bp ? bp[(long)iu * ldb] : 0.0;
                a[u] = alpha ? alpha[iu] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double kk = exp_gauss(gauss_q<D>(p, q[u], g));
                const double kb = kk * b[u], ka = kk * a[u];
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double e = q[u][k] - p[k];
                    sv[k] = fma(kb, e, sv[k]);
                    sm[k] = fma(ka, e, sm[k]);
                }
            }
        }
        for (; i < n; i += 64) {
            double q[D];
#pragma unroll
            for (int k = 0; k < D; ++k)
                q[k] = x[k + (long)i * D];
            const double kk = exp_gauss(gauss_q<D>(p, q, g));
            const double kb = kk * (bp ? bp[(long)i * ldb] : 0.0);
            const double ka = kk * (alpha ? alpha[i] : 0.0);
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double e = q[k] - p[k];
                sv[k] = fma(kb, e, sv[k]);
                sm[k] = fma(ka, e, sm[k]);
            }
        }
    }
    // the four slices of a row within the wave (lanes r, r + 16, r + 32, r + 48), then the waves
    __shared__ double part[16][2 * D][16];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        sv[k] += __shfl_down(sv[k], 32, 64);
        sv[k] += __shfl_down(sv[k], 16, 64);
        sm[k] += __shfl_down(sm[k], 32, 64);
        sm[k] += __shfl_down(sm[k], 16, 64);
    }
    if ((t & 63) < 16) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            part[wave][k][r] = sv[k];
            part[wave][D + k][r] = sm[k];
        }
    }
    __syncthreads();
    if (t < 2 * D * 16 && row < m) {
        const int qn = t >> 4; // which sum: dvar's D, then dmean's D
        double s = 0.0;
        for (int w = 0; w < 16; ++w)
            s += part[w][qn][r];
        if (qn < D) {
            if (dvar)
                dvar[qn + (long)row * D] = -2.0 * (g.c * (-2.0 * g.nh[qn])) * s;
        } else if (dmean) {
            dmean[qn - D + (long)row * D] = (g.c * (-2.0 * g.nh[qn - D])) * s;
        }
    }
}

// The mean and its gradient without a sweep: predict_mean_kernel (one wave per query point, lanes
// stride over i, one exponential per pair) with D more accumulators and the same shuffle tree for
// each.  dmean: d x M, entry [k + j d].
template <int D>
__global__ __launch_bounds__(256) void predict_mean_grad_kernel(const double *__restrict__ xo,
                                                                int M,
                                                                const double *__restrict__ x, int n,
                                                                const double *__restrict__ alpha,
                                                                GaussParams g,
                                                                double *__restrict__ mean,
                                                                double *__restrict__ dmean)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    if (i >= M)
        return;
    double p[D], sg[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        p[k] = xo[k + (long)i * D];
        sg[k] = 0.0;
    }
    double s = 0.0;
    for (int j = lane; j < n; j += 64) {
        double q[D];
#pragma unroll
        for (int k = 0; k < D; ++k)
            q[k] = x[k + (long)j * D];
        const double ka = exp_gauss(gauss_q<D>(p, q, g)) * alpha[j];
        s += ka;
#pragma unroll
        for (int k = 0; k < D; ++k)
            sg[k] = fma(ka, q[k] - p[k], sg[k]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
#pragma unroll
        for (int k = 0; k < D; ++k)
            sg[k] += __shfl_down(sg[k], off, 64);
    }
    if (lane == 0) {
        if (mean)
            mean[i] = g.c * s;
#pragma unroll
        for (int k = 0; k < D; ++k)
            dmean[k + (long)i * D] = (g.c * (-2.0 * g.nh[k])) * sg[k];
    }
}
