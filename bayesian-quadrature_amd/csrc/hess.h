// hess.h -- the Hessian of a resident fit's log marginal likelihood (bq_gp_logml_hess, fit.hip).
//
// With K = K0 + s^2 I, Ki = K^-1 = Y Y^T (Y = L^-T, kept by the gradient), a = Ki y,
// G = a a^T - Ki, u_k = r_k^2 / w_k^3 - 1 / w_k and D_h = 2 K0 / h, D_k = K0 o u_k, D_s = 2 s I:
//   H_pq = 1/2 sum(G o D_pq) - (D_p a)^T Ki (D_q a) + 1/2 tr(Ki D_p Ki D_q)
// Ki D_h = (2 / h) C with C = I - s^2 Ki and Ki D_s = 2 s Ki need no product; B_k = Ki D_k is the
// one n x n x n product per length scale.  Its D_k operand is generated from the resident points
// chunk by chunk, never stored (dk.h: its entries and the rows of D_k a; wgsum.h: the workgroup's
// fixed-order sums and fold_kernel, which folds the tiles' partials).
//
//   hess_prod_kernel<0>    Ki = Y Y^T, all of it (a tile's k range starts at its first row or
//                          column, whichever is later: Y is upper triangular)
//   hess_prod_kernel<D>    B_k = Ki D_k
//   hess_gsum_kernel<D>    the D_pq-weighted sums over G, per 64 x 64 tile
//   hess_trace_kernel<D>   the elementwise sums that are the traces, per 64 x 64 tile
//   hess_dka_kernel<D>     the vectors D_p a
//   hess_kiv_kernel        Ki (D_p a)
//   hess_quad_kernel       the dot products (D_p a)^T Ki (D_q a), p <= q
// Rows and columns at or beyond n (the identity padding) are masked out of every sum.
#pragma once
#include "common.h"
#include "dk.h"
#include "wgsum.h"

// C (npad x npad, ld npad) = A Q^T over k in [0, npad).
// D == 0: Q is a matrix like A (both Y = L^-T: C = Ki); the k range starts at max(R0, C0).
// D > 0: A = Ki and Q(j, k) = D_kdim(j, k) = K0(j, k) u_kdim(j, k), generated (C = B_kdim).
// Workgroup: 4 waves as WR x WC, wave tile 16 TM x 16 TN, v_mfma_f64_16x16x4; a chunk of 16 k
// columns of both operands goes through registers into LDS (the loads and the exp of chunk c + 1
// are issued before the MFMAs of chunk c).  The generated operand costs one exp per entry and
// k column of the workgroup tile's column range: the tall 256 x 64 tile spends a quarter of the
// 64 x 64 tile's on it and takes the large systems.  (Two workgroups per CU at the least: the
// tall tile's 64 accumulator registers otherwise leave a SIMD one wave and nothing to hide a
// barrier behind.)
template <int D, int WR, int WC, int TM, int TN>
__global__ __launch_bounds__(256, 2) void hess_prod_kernel(double *__restrict__ C,
                                                        const double *__restrict__ A,
                                                        const double *__restrict__ Q, HessJob hj,
                                                        int kdim)
{
    static_assert(WR * WC == 4, "four waves");
    constexpr int ROWS = WR * TM * 16, COLS = WC * TN * 16;
    static_assert(COLS == 64, "the generated operand is dealt as 64 columns x 4 k rows");
    // (row strides of 16 mod 32 doubles: the four k rows of a fragment read fall in disjoint banks)
    constexpr int LDA = ROWS + 16, LDQ = COLS + 16;
    constexpr int NA = ROWS * BQ_DK_KC / 256, NQ = COLS * BQ_DK_KC / 256;
    __shared__ double sA[BQ_DK_KC * LDA];
    __shared__ double sQ[BQ_DK_KC * LDQ];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int npad = hj.npad;
    const long ld = npad;
    const int R0 = blockIdx.x * ROWS, C0 = blockIdx.y * COLS;
    const int wr0 = (wave % WR) * TM * 16, wc0 = (wave / WR) * TN * 16;

    // the generated operand: this thread's column j and its coordinates, for every chunk
    const int jq = C0 + (t & 63), kq = t >> 6;
    double xj[D > 0 ? D : 1];
    double iw = 0.0, iw2 = 0.0;
    if constexpr (D > 0) {
#pragma unroll
        for (int k = 0; k < D; ++k)
            xj[k] = jq < hj.n ? hj.pts[k + (long)jq * D] : 0.0;
        iw = hj.iw[kdim];
        iw2 = iw * iw;
    }

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
            const int idx = t + 256 * e, i = idx % ROWS, kk = idx / ROWS;
            ra[e] = A[min(R0 + i, npad - 1) + (long)(k0 + kk) * ld];
        }
        if constexpr (D == 0) {
#pragma unroll
            for (int e = 0; e < NQ; ++e)
                rq[e] = Q[jq + (long)(k0 + kq + 4 * e) * ld];
        } else {
#pragma unroll
            for (int e = 0; e < NQ; ++e) {
                const int k = k0 + kq + 4 * e;
                double v = 0.0;
                if (jq < hj.n && k < hj.n) {
                    double r2[D], rk = 0.0;
                    const double k0v = gauss_k0<D>(xj, hj.pts + (long)k * D, hj.g, r2);
#pragma unroll
                    for (int m = 0; m < D; ++m)
                        rk = m == kdim ? r2[m] : rk;
                    v = k0v * dk_weight(iw, iw2, rk);
                }
                rq[e] = v;
            }
        }
    };

    int kbeg = 0;
    if constexpr (D == 0) // Y(i, k) = 0 for k < i
        kbeg = max(R0, C0) & ~(BQ_DK_KC - 1);
    const int kend = D == 0 ? npad : (int)((hj.n + BQ_DK_KC - 1) & ~(BQ_DK_KC - 1));
    if (kbeg < kend)
        fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += BQ_DK_KC) {
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
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int r = R0 + wr0 + 16 * tm;
        if (r >= npad)
            continue; // (a tall tile's last rows; npad is a multiple of 64)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                C[(r + l15) + (long)(C0 + wc0 + 16 * tn + 4 * rr + l4) * ld] = acc[tm][tn][rr];
    }
}

// One workgroup's NC sums (wg_wave_sums, wgsum.h) into part: [NC][nwg], this workgroup's column wg
template <int NC>
__device__ __forceinline__ void hess_block_sums(double (&sum)[NC], double *red,
                                                double *__restrict__ part, int wg, int nwg)
{
    const double v = wg_wave_sums<NC>(sum, red, threadIdx.x & 63, threadIdx.x >> 6);
    if (threadIdx.x < NC)
        part[(long)threadIdx.x * nwg + wg] = v;
}

// The sums of G = a a^T - Ki against K0 and its weights, one 64 x 64 tile per workgroup
// (grid: npad / 64 squared); hess_ng(D) partials per workgroup
template <int D>
__global__ __launch_bounds__(256) void hess_gsum_kernel(const double *__restrict__ Ki, HessJob hj,
                                                        double *__restrict__ part)
{
    constexpr int NC = hess_ng(D);
    __shared__ double red[4 * NC];
    double sum[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
        sum[c] = 0.0;
    const int t = threadIdx.x;
    const int i = blockIdx.x * 64 + (t & 63);
    const long ld = hj.npad;
    if (i < hj.n) {
        double xi[D], iw[D], iw2[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            xi[k] = hj.pts[k + (long)i * D];
            iw[k] = hj.iw[k];
            iw2[k] = iw[k] * iw[k];
        }
        const double ai = hj.alpha[i];
        for (int e = 0; e < 16; ++e) {
            const int j = blockIdx.y * 64 + (t >> 6) + 4 * e;
            if (j >= hj.n)
                continue;
            const double G = ai * hj.alpha[j] - Ki[i + j * ld];
            double r2[D], u[D];
            const double gk = G * gauss_k0<D>(xi, hj.pts + (long)j * D, hj.g, r2);
            sum[0] += gk;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                u[k] = dk_weight(iw[k], iw2[k], r2[k]);
                sum[1 + k] += gk * u[k];
            }
#pragma unroll
            for (int k = 0; k < D; ++k)
#pragma unroll
                for (int l = k; l < D; ++l) {
                    double wkl = u[k] * u[l];
                    if (l == k) // + 1 / w^2 - 3 r^2 / w^4
                        wkl += iw2[k] * (1.0 - 3.0 * (iw2[k] * r2[k]));
                    sum[1 + D + hess_pair(D, k, l)] += gk * wkl;
                }
            if (i == j)
                sum[NC - 1] += G;
        }
    }
    hess_block_sums<NC>(sum, red, part, blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
}

// The traces as elementwise sums, with C = I - s^2 Ki (Ki and C are symmetric, B_k is not):
// tile (I, J) of Ki and of every B_k against tile (J, I) of every B_l, which comes through LDS
// transposed.  B: the d products, npad^2 apart.  hess_nt(D) partials per workgroup.
template <int D>
__global__ __launch_bounds__(256) void hess_trace_kernel(const double *__restrict__ Ki,
                                                         const double *__restrict__ B, HessJob hj,
                                                         double *__restrict__ part)
{
    constexpr int NC = hess_nt(D);
    __shared__ double red[4 * NC];
    __shared__ double sT[64 * 65];
    double sum[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
        sum[c] = 0.0;
    const int t = threadIdx.x, il = t & 63, jl0 = t >> 6;
    const int I0 = blockIdx.x * 64, J0 = blockIdx.y * 64;
    const int i = I0 + il;
    const long ld = hj.npad, bs = ld * ld;
    const bool rowin = i < hj.n;
    if (rowin)
        for (int e = 0; e < 16; ++e) {
            const int j = J0 + jl0 + 4 * e;
            if (j >= hj.n)
                continue;
            const double kij = Ki[i + j * ld];
            const double cij = (i == j ? 1.0 : 0.0) - hj.g.s2 * kij;
            sum[0] += cij * cij;
            sum[1] += cij * kij;
            sum[2] += kij * kij;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double b = B[k * bs + i + j * ld];
                sum[3 + k] += cij * b;
                sum[3 + D + k] += kij * b;
            }
        }
#pragma unroll
    for (int l = 0; l < D; ++l) {
        __syncthreads();
        // B_l(J0 + il, I0 + c) -> sT[c][il]
        for (int e = 0; e < 16; ++e) {
            const int c = jl0 + 4 * e;
            sT[c * 65 + il] = B[l * bs + (J0 + il) + (I0 + c) * ld];
        }
        __syncthreads();
        if (rowin)
            for (int e = 0; e < 16; ++e) {
                const int jl = jl0 + 4 * e;
                if (J0 + jl >= hj.n)
                    continue;
                const double bt = sT[il * 65 + jl]; // B_l(j, i)
#pragma unroll
                for (int k = 0; k <= l; ++k)
                    sum[3 + 2 * D + hess_pair(D, k, l)] += B[k * bs + i + (J0 + jl) * ld] * bt;
            }
    }
    hess_block_sums<NC>(sum, red, part, blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
}

// V[p] = D_p a, p over [h, w_1 .. w_d, s], npad apart: D_h a = (2 / h)(y - s^2 a), D_s a = 2 s a,
// D_k a from the generated operand -- 16 rows per workgroup, a row's columns dealt to 16 lanes
// and summed by shuffles.  Rows at or beyond n are zero.  grid: npad / 16
template <int D>
__global__ __launch_bounds__(256) void hess_dka_kernel(HessJob hj, const double *__restrict__ y,
                                                       double two_over_h, double two_s,
                                                       double *__restrict__ V)
{
    const int t = threadIdx.x, i = blockIdx.x * 16 + (t >> 4), jl = t & 15;
    double sum[D];
    dka_sums<D>(hj, i, jl, sum);
    if (jl == 0) {
        const long ld = hj.npad;
        const bool in = i < hj.n;
        const double a = in ? hj.alpha[i] : 0.0;
        V[i] = in ? two_over_h * (y[i] - hj.g.s2 * a) : 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k)
            V[(1 + k) * ld + i] = sum[k];
        V[(D + 1) * ld + i] = two_s * a;
    }
}

// Z[p] = Ki V[p] for the np vectors: a wave per column i of the symmetric Ki, four per workgroup.
// grid: npad / 4
__global__ __launch_bounds__(256) void hess_kiv_kernel(const double *__restrict__ Ki, int n,
                                                       int npad, int np,
                                                       const double *__restrict__ V,
                                                       double *__restrict__ Z)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    double sum[BQ_MAXD + 2];
#pragma unroll
    for (int p = 0; p < BQ_MAXD + 2; ++p)
        sum[p] = 0.0;
    if (i < n)
        for (int k = lane; k < n; k += 64) {
            const double kv = Ki[k + (long)i * npad];
#pragma unroll
            for (int p = 0; p < BQ_MAXD + 2; ++p)
                if (p < np)
                    sum[p] += kv * V[(long)p * npad + k];
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int p = 0; p < BQ_MAXD + 2; ++p)
            sum[p] += __shfl_xor(sum[p], off);
    if (lane == 0)
#pragma unroll
        for (int p = 0; p < BQ_MAXD + 2; ++p)
            if (p < np)
                Z[(long)p * npad + i] = sum[p];
}

// out[pair(p, q)] = V[p] . Z[q], p <= q < np, one workgroup, fixed order
__global__ __launch_bounds__(256) void hess_quad_kernel(const double *__restrict__ V,
                                                        const double *__restrict__ Z, int n,
                                                        int npad, int np, double *__restrict__ out)
{
    __shared__ double red[256];
    const int t = threadIdx.x;
    int o = 0;
    for (int p = 0; p < np; ++p)
        for (int q = p; q < np; ++q, ++o) {
            double v = 0.0;
            for (int i = t; i < n; i += 256)
                v += V[(long)p * npad + i] * Z[(long)q * npad + i];
            // (wgsum.h's tree, written out: through wg_tree_sum the kernel compiles differently)
            red[t] = v;
            __syncthreads();
            for (int h = 128; h > 0; h >>= 1) {
                if (t < h)
                    red[t] += red[t + h];
                __syncthreads();
            }
            if (t == 0)
                out[o] = red[0];
            __syncthreads();
        }
}
