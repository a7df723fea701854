// ptheta.h -- derivatives of the posterior mean and variance with respect to the hyper-parameters
// theta = [h, w_1 .. w_d, s] (bq_gp_predict_dtheta, fit.hip).  Compiled into k_hess.hip (host.h
// lists the units); dk.h has the derivative operand's entries and the rows of D_k a, which the
// Hessian shares.
//
// With K = K0 + s^2 I, Ki = K^-1, a = Ki y, k_ji = k(xo_j, x_i), beta_j = Ki k_j, k0 = k(x, x),
// D_k = K0 o (r_k^2 / w_k^3 - 1 / w_k), g_jik = (xo_jk - x_ik)^2 / w_k^3 - 1 / w_k, and the solved
// vectors u = Ki a, z_k = Ki (D_k a), which depend on the fit alone (bq_fit::DKZ):
//   d mean_j / d h   =  (2 s^2 / h) sum_i k_ji u_i
//   d mean_j / d w_k =  sum_i k_ji g_jik a_i - sum_i k_ji z_k,i
//   d mean_j / d s   = -2 s sum_i k_ji u_i
//   d var_j  / d h   =  (2 / h) (var_j - s^2 |beta_j|^2)
//   d var_j  / d w_k = -k0 / w_k - 2 sum_i k_ji g_jik beta_ji + q_jk,   q_jk = beta_j^T D_k beta_j
//   d var_j  / d s   =  2 s |beta_j|^2
// The h and s rows hold no difference of large terms, and at s = 0 the h row of dmean and the s rows
// of both are products with an exact zero.
//
//   ptheta_dka_kernel<D>          the right-hand sides [a, D_1 a .. D_d a] as rows for the row sweeps
//   ptheta_quad_kernel<D, ..>     q_jk per 64-column block: beta D_k on the MFMAs, the tile reduced
//                                 against beta in the epilogue, never stored
//   predict_theta_kernel<D>       the M x n row sums and the finished derivatives
//   predict_mean_theta_kernel<D>  the mean and its derivatives alone, a wave per query point
// Determinism as in reduce.h, hess.h and pgrad.h: every sum has a fixed order (a thread's columns
// in sequence, a shuffle tree, partials in index order) and there are no atomics.  Padding rows,
// columns and points are never read into a sum; indices are clamped, values masked.
#pragma once
#include "common.h"
#include "dk.h"

// R (64 x npad, ld 64, point i in column i): row 0 = a, row 1 + k = D_k a, the other rows and the
// columns at or beyond n zero -- the shape the row sweeps take (R Ki = [u, z_1 .. z_d] as rows).
// 16 points per workgroup, 16 lanes per point (dka_sums, dk.h).  grid: npad / 16
template <int D>
__global__ __launch_bounds__(256) void ptheta_dka_kernel(HessJob hj, double *__restrict__ R)
{
    const int t = threadIdx.x, i = blockIdx.x * 16 + (t >> 4), jl = t & 15;
    const bool in = i < hj.n;
    double sum[D];
    dka_sums<D>(hj, i, jl, sum);
    // every lane of the point holds the sums: lane jl writes rows jl, jl + 16, jl + 32, jl + 48
    const double a = in ? hj.alpha[i] : 0.0;
#pragma unroll
    for (int e = 0; e < BQ_PTHETA_ROWS / 16; ++e) {
        const int p = jl + 16 * e;
        double v = p == 0 ? a : 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k)
            v = p == 1 + k ? sum[k] : v;
        R[p + (long)BQ_PTHETA_ROWS * i] = in ? v : 0.0;
    }
}

// part[kdim][column block][row] = sum over the block's columns i < n of T(row, i) beta(row, i),
// T = beta D_kdim -- the q_jk of one length scale, in npad / 64 pieces per row that the finishing
// kernel adds in index order.  beta: Mp x npad, ld = ldb, rows along the fast index (what the
// backward row sweep leaves).  hess_prod_kernel<D>'s structure, written out in both (dk.h says why):
// four waves as WR x WC on v_mfma_f64_16x16x4, wave tile 16 TM x 16 TN, 16-deep k chunks of both
// operands through registers into LDS, the D_k entries of chunk c + 1 generated from the points
// (gauss_k0, dk_weight) while the MFMAs of chunk c run, k < n and column < n masked.  What differs: the left operand has Mp rows and its own
// ld (rows clamped to Mp - 1, k columns at or beyond n read as zero); T is never stored -- the
// epilogue multiplies the accumulators by the matching beta, sums a row's 64 columns in a fixed
// order (a lane's 4 TN entries in sequence, the four 16-lane groups by two shuffles, the WC waves
// through LDS in index order) and writes one partial per row.  The tall 256 x 64 tile spends a
// quarter of the 64 x 64 tile's exponentials (k_hess.hip, ptheta_tall, has the rule).
// grid: (ceil(Mp / ROWS), npad / 64)
template <int D, int WR, int WC, int TM, int TN>
__global__ __launch_bounds__(256, 2) void ptheta_quad_kernel(const double *__restrict__ beta,
                                                             long ldb, int Mp, HessJob hj, int kdim,
                                                             double *__restrict__ part)
{
    static_assert(WR * WC == 4, "four waves");
    constexpr int ROWS = WR * TM * 16, COLS = WC * TN * 16;
    static_assert(COLS == 64, "the generated operand is dealt as 64 columns x 4 k rows");
    static_assert(ROWS <= 256, "a thread per row folds the waves");
    constexpr int LDA = ROWS + 16, LDQ = COLS + 16;
    constexpr int NA = ROWS * BQ_DK_KC / 256, NQ = COLS * BQ_DK_KC / 256;
    __shared__ double sA[BQ_DK_KC * LDA];
    __shared__ double sQ[BQ_DK_KC * LDQ];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int n = hj.n;
    const int R0 = blockIdx.x * ROWS, C0 = blockIdx.y * COLS;
    const int wr0 = (wave % WR) * TM * 16, wc0 = (wave / WR) * TN * 16;

    // the generated operand: this thread's column j and its coordinates, for every chunk
    const int jq = C0 + (t & 63), kq = t >> 6;
    double xj[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        xj[k] = jq < n ? hj.pts[k + (long)jq * D] : 0.0;
    const double iw = hj.iw[kdim], iw2 = iw * iw;

    double4_t acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = (double4_t){0.0, 0.0, 0.0, 0.0};

    double ra[NA], rq[NQ];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < NA; ++e) {
            const int idx = t + 256 * e, i = idx % ROWS, k = k0 + idx / ROWS;
            const double v = beta[min(R0 + i, Mp - 1) + (long)min(k, n - 1) * ldb];
            ra[e] = k < n ? v : 0.0;
        }
#pragma unroll
        for (int e = 0; e < NQ; ++e) {
            const int k = k0 + kq + 4 * e;
            double v = 0.0;
            if (jq < n && k < n) {
                double r2[D], rk = 0.0;
                const double k0v = gauss_k0<D>(xj, hj.pts + (long)k * D, hj.g, r2);
#pragma unroll
                for (int m = 0; m < D; ++m)
                    rk = m == kdim ? r2[m] : rk;
                v = k0v * dk_weight(iw, iw2, rk);
            }
            rq[e] = v;
        }
    };

    const int kend = (n + BQ_DK_KC - 1) & ~(BQ_DK_KC - 1);
    fetch(0);
    for (int k0 = 0; k0 < kend; k0 += BQ_DK_KC) {
        __syncthreads(); // every wave is done with the chunk before
#pragma unroll
        for (int e = 0; e < NA; ++e) {
            const int idx = t + 256 * e;
            sA[(idx / ROWS) * LDA + idx % ROWS] = ra[e];
        }
#pragma unroll
        for (int e = 0; e < NQ; ++e)
            sQ[(kq + 4 * e) * LDQ + (t & 63)] = rq[e];
        __syncthreads();
        if (k0 + BQ_DK_KC < kend)
            fetch(k0 + BQ_DK_KC);
#pragma unroll
        for (int ks = 0; ks < BQ_DK_KC / 4; ++ks) {
            double fa[TM], fq[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
                fa[tm] = sA[(4 * ks + l4) * LDA + wr0 + 16 * tm + l15];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                fq[tn] = sQ[(4 * ks + l4) * LDQ + wc0 + 16 * tn + l15];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(fq[tn], fa[tm], acc[tm][tn],
                                                                       0, 0, 0);
        }
    }
    // register rr of block (tm, tn): row 16 tm + l15, column 16 tn + 4 rr + l4
    double rs[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int r = min(R0 + wr0 + 16 * tm + l15, Mp - 1);
        double s = 0.0;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int col = C0 + wc0 + 16 * tn + 4 * rr + l4;
                const double b = beta[r + (long)min(col, n - 1) * ldb];
                s += col < n ? acc[tm][tn][rr] * b : 0.0;
            }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        rs[tm] = s;
    }
    __syncthreads(); // sA is free: the waves' row sums, [wave column][row]
    double *red = sA;
    if (l4 == 0)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
            red[(wave / WR) * ROWS + wr0 + 16 * tm + l15] = rs[tm];
    __syncthreads();
    if (t < ROWS && R0 + t < Mp) {
        double s = red[t];
#pragma unroll
        for (int wc = 1; wc < WC; ++wc)
            s += red[wc * ROWS + t];
        part[((long)kdim * gridDim.y + blockIdx.y) * Mp + R0 + t] = s;
    }
}

// the constants that multiply the finished sums
struct ThetaScale {
    double two_s2_over_h, neg_two_s; // dmean: the h and s rows against c sum k u
    double two_over_h, two_s;        // dvar: the h and s rows
};

// The M x n sums and the finished derivatives.  predict_grad_kernel<D>'s decomposition -- 16 rows x
// column slices per workgroup, a thread keeps its query point in registers and recomputes k_ji
// with exp_gauss over gauss_q's arithmetic (the cross Gram is gone by now), a shuffle tree, then
// the waves through LDS in index order -- with 512 threads, 32 column slices: a row carries up to
// 3 D + 2 sums (sum k u; sum k g_k a, sum k z_k, sum k g_k beta per length scale; sum beta^2), 26 at
// D = 8, which beside the query point and one training point do not fit the 128 registers of a
// 1024-thread block; 512 threads have 256, and one kernel keeps one exponential per pair for both
// parts.  The sums leave the constant c out; it and 2 / h, 2 s .. multiply the finished sums.
//   beta   Mp x npad, ld = ldb (the backward row sweep's); read only for dvar
//   Z      64 x npad, ld 64: [u, z_1 .. z_d] as rows (bq_fit::DKZ); read only for dmean
//   var    the row's posterior variance (bq_gp_predict's), qpart the quad kernel's partials
//          ([D][ncb][ldq]), added here in index order
//   dmean, dvar   (D + 2) x m, entry [p + row (D + 2)], p over [h, w_1 .. w_D, s]; nullptr: that
//          part is off and its operands are not read
// Only i < n and row < m are read or summed.  xo may be mapped host memory.  grid: ceil(m / 16).
// LDS: 8 waves x (3 D + 2) x 16 rows of partial sums (26 KB at D = 8).
template <int D>
__global__ __launch_bounds__(512) void predict_theta_kernel(const double *__restrict__ beta, long ldb,
                                                            int m, const double *__restrict__ xo,
                                                            HessJob hj, const double *__restrict__ Z,
                                                            const double *__restrict__ var,
                                                            const double *__restrict__ qpart,
                                                            int ncb, long ldq, ThetaScale sc,
                                                            double *__restrict__ dmean,
                                                            double *__restrict__ dvar)
{
    constexpr int NS = 3 * D + 2; // su | sga[D] | sz[D] | sbb | sgb[D]
    const int t = threadIdx.x, r = t & 15, sl = t >> 4, wave = t >> 6;
    const int row = blockIdx.x * 16 + r;
    const bool live = row < m;
    const int n = hj.n;
    double p[D], iw[D], iw2[D], S[NS];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        p[k] = live ? xo[k + (long)row * D] : 0.0;
        iw[k] = hj.iw[k];
        iw2[k] = iw[k] * iw[k];
    }
#pragma unroll
    for (int c = 0; c < NS; ++c)
        S[c] = 0.0;
    if (live) {
        const double *bp = dvar ? beta + row : nullptr;
        const double *zp = dmean ? Z : nullptr;
#pragma unroll 2
        for (int i = sl; i < n; i += 32) {
            double gk[D], qq = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double tt = p[k] - hj.pts[k + (long)i * D];
                const double r2 = tt * tt;
                qq += r2 * hj.g.nh[k];
                gk[k] = dk_weight(iw[k], iw2[k], r2);
            }
            const double kk = exp_gauss(qq);
            if (zp) {
                const double *zi = zp + (long)BQ_PTHETA_ROWS * i;
                const double ka = kk * hj.alpha[i];
                S[0] = fma(kk, zi[0], S[0]);
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    S[1 + k] = fma(ka, gk[k], S[1 + k]);
                    S[1 + D + k] = fma(kk, zi[1 + k], S[1 + D + k]);
                }
            }
            if (bp) {
                const double b = bp[(long)i * ldb], kb = kk * b;
                S[1 + 2 * D] = fma(b, b, S[1 + 2 * D]);
#pragma unroll
                for (int k = 0; k < D; ++k)
                    S[2 + 2 * D + k] = fma(kb, gk[k], S[2 + 2 * D + k]);
            }
        }
    }
    // the four slices of a row within the wave (lanes r, r + 16, r + 32, r + 48), then the waves
    __shared__ double part[8][NS][16];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        S[c] += __shfl_down(S[c], 32, 64);
        S[c] += __shfl_down(S[c], 16, 64);
    }
    if ((t & 63) < 16) {
#pragma unroll
        for (int c = 0; c < NS; ++c)
            part[wave][c][r] = S[c];
    }
    __syncthreads();
    // a thread per output: (which, p, row), which = 0 dmean, 1 dvar
    const int o = t >> 4, which = o / (D + 2), pp = o % (D + 2);
    if (which < 2 && live && (which ? dvar != nullptr : dmean != nullptr)) {
        auto total = [&](int c) {
            double s = 0.0;
            for (int w = 0; w < 8; ++w)
                s += part[w][c][r];
            return s;
        };
        const double c0 = hj.g.c;
        double v;
        if (which == 0) {
            if (pp == 0)
                v = sc.two_s2_over_h * (c0 * total(0));
            else if (pp == D + 1)
                v = sc.neg_two_s * (c0 * total(0));
            else
                v = c0 * total(pp) - c0 * total(D + pp);
            dmean[pp + (long)row * (D + 2)] = v;
        } else {
            if (pp == 0)
                v = sc.two_over_h * (var[row] - hj.g.s2 * total(1 + 2 * D));
            else if (pp == D + 1)
                v = sc.two_s * total(1 + 2 * D);
            else {
                const int k = pp - 1;
                double q = 0.0;
                for (int cb = 0; cb < ncb; ++cb)
                    q += qpart[((long)k * ncb + cb) * ldq + row];
                v = (-c0 * iw[k] - 2.0 * (c0 * total(2 + 2 * D + k))) + q;
            }
            dvar[pp + (long)row * (D + 2)] = v;
        }
    }
}

// The mean and its derivatives without a sweep: predict_mean_grad_kernel<D>'s shape (one wave per
// query point, lanes stride over i, one exponential per pair) with 2 D + 1 more accumulators and
// the same shuffle tree for each.  Z as above; dmean: (D + 2) x M, entry [p + j (D + 2)].
template <int D>
__global__ __launch_bounds__(256) void predict_mean_theta_kernel(const double *__restrict__ xo, int M,
                                                                 HessJob hj,
                                                                 const double *__restrict__ Z,
                                                                 ThetaScale sc,
                                                                 double *__restrict__ mean,
                                                                 double *__restrict__ dmean)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    if (i >= M)
        return;
    double p[D], iw[D], iw2[D], sga[D], sz[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        p[k] = xo[k + (long)i * D];
        iw[k] = hj.iw[k];
        iw2[k] = iw[k] * iw[k];
        sga[k] = 0.0;
        sz[k] = 0.0;
    }
    double s = 0.0, su = 0.0;
    for (int j = lane; j < hj.n; j += 64) {
        double gk[D], qq = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double tt = p[k] - hj.pts[k + (long)j * D];
            const double r2 = tt * tt;
            qq += r2 * hj.g.nh[k];
            gk[k] = dk_weight(iw[k], iw2[k], r2);
        }
        const double kk = exp_gauss(qq), ka = kk * hj.alpha[j];
        const double *zj = Z + (long)BQ_PTHETA_ROWS * j;
        s += ka;
        su = fma(kk, zj[0], su);
#pragma unroll
        for (int k = 0; k < D; ++k) {
            sga[k] = fma(ka, gk[k], sga[k]);
            sz[k] = fma(kk, zj[1 + k], sz[k]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
        su += __shfl_down(su, off, 64);
#pragma unroll
        for (int k = 0; k < D; ++k) {
            sga[k] += __shfl_down(sga[k], off, 64);
            sz[k] += __shfl_down(sz[k], off, 64);
        }
    }
    if (lane == 0) {
        const double c0 = hj.g.c;
        if (mean)
            mean[i] = c0 * s;
        double *o = dmean + (long)i * (D + 2);
        o[0] = sc.two_s2_over_h * (c0 * su);
#pragma unroll
        for (int k = 0; k < D; ++k)
            o[1 + k] = c0 * sga[k] - c0 * sz[k];
        o[D + 1] = sc.neg_two_s * (c0 * su);
    }
}
