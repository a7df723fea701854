// lgo.h -- leave-group-out cross-validation of a resident fit (bq_gp_lgo, bq_gp_lgo_grad, fit.hip).
//
// With P = Kxx^-1 = Y Y^T (Y = L^-T), a = P y and a group B of b <= BQ_LGO_MAX indices:
//   Sigma_B = (P_BB)^-1,  r_B = Sigma_B a_B,  mu_B = y_B - r_B,  cov_B = Sigma_B
//   lp_B = 1/2 log|P_BB| - 1/2 a_B.r_B - (b / 2) log 2 pi,  L_lgo = sum_B lp_B
//   d lp_B / d theta_p = r_B.v_p - 1/2 r_B^T M_p r_B - 1/2 tr(Sigma_B M_p)
// with v_p = (P D_p a)_B, the Hessian's resident vectors (hess.h), and M_p = (P D_p P)_BB:
//   M_h = (2 / h)(P_BB - s^2 Q_BB),  M_k = (B_k P)_BB,  M_s = 2 s Q_BB,  Q = P P,  B_k = P D_k
// Since tr(Sigma_B P_BB) = b and r_B^T P_BB r_B = a_B.r_B, the h entry needs Q_BB only.  With
// b = 1 these are loo.h's formulas.
//
//   lgo_block_kernel<MODE, BT>  the groups' b x b blocks of one product, partial over a chunk of
//                               columns: P_BB from Y (LGO_YY), Q_BB (LGO_PP), the M_k (LGO_BP).
//                               A workgroup takes a bundle: consecutive groups of at most 64
//                               members together (the host packs them), multiplies their rows
//                               as one block and keeps the entries inside a group -- 64
//                               singletons cost one pass over the matrix, not 64
//   lgo_group_kernel            per group: the chunks' partials of P_BB in their order, its
//                               Cholesky factor C, r_B by two solves, Sigma_B = C^-T C^-1, mu,
//                               diag Sigma_B, lp
//   lgo_group_grad_kernel       per group: the d + 2 gradient entries from Sigma_B, r_B and the
//                               partials of Q_BB and the M_k
// The groups' lp, and their gradient entries, are summed in group order by wgsum.h's fold_kernel
// (launched from k_hess.hip).
// loo.h's rules: no atomics, every sum in a fixed order (the same bits on every call), rows and
// columns at or beyond n stay out of every sum.  A block is stored as b rows of 64 doubles: member
// t of the flattened index list owns row t, so the blocks of all groups are T x 64 per chunk.
#pragma once
#include "common.h"
#include "loo.h"
#include "wgsum.h"

#define BQ_LGO_MAXB 64 // = BQ_LGO_MAX (bqhip.h)
#define BQ_LGO_SLAB 32 // columns staged in LDS at a time
#define BQ_LGO_LD 65   // row stride of a staged slab: the column-wise fill hits every bank

enum { LGO_YY = 0, LGO_PP = 1, LGO_BP = 2 };

// slab[mm][i] = M(gi[i], m0 + mm): rows of a column-major matrix (a wave reads one column, 64
// scattered rows).  tri: M is upper triangular and what lies below its diagonal is not read.
__device__ __forceinline__ void lgo_stage_rows(const double *__restrict__ M, int npad, const int *gi,
                                               int b, int m0, int cend, bool tri, double *slab)
{
    const int i = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < BQ_LGO_SLAB / 4; ++k) {
        const int mm = w + 4 * k, m = m0 + mm;
        double v = 0.0;
        if (i < b && m < cend && (!tri || m >= gi[i]))
            v = M[gi[i] + (long)m * npad];
        slab[mm * BQ_LGO_LD + i] = v;
    }
}

// slab[mm][i] = M(m0 + mm, gi[i]): columns of a column-major matrix (32 consecutive doubles each)
__device__ __forceinline__ void lgo_stage_cols(const double *__restrict__ M, int npad, const int *gi,
                                               int b, int m0, int cend, double *slab)
{
#pragma unroll
    for (int k = 0; k < BQ_LGO_SLAB / 4; ++k) {
        const int e = threadIdx.x + 256 * k, mm = e & (BQ_LGO_SLAB - 1), i = e / BQ_LGO_SLAB;
        const int m = m0 + mm;
        double v = 0.0;
        if (i < b && m < cend)
            v = M[m + (long)gi[i] * npad];
        slab[mm * BQ_LGO_LD + i] = v;
    }
}

// One product's blocks of the groups [bundle[blockIdx.x], bundle[blockIdx.x + 1]), b members in
// all, over the columns [chunk cw, (chunk + 1) cw) below n; i, j run over the bundle's members:
//   LGO_YY  sum_m A(i, m) A(j, m), A = Y upper triangular     (P is not read)
//   LGO_PP  sum_m P(m, i) P(m, j)                             (A is not read)
//   LGO_BP  sum_m A_z(i, m) P(m, j), A_z = A + z npad^2, z = blockIdx.z, into product 1 + z
// Thread (ti, tj) of 16 x 16 owns the entries (ti + 16 a, tj + 16 c), a, c < BT; BT = 1, 2, 4 for
// a launch whose largest bundle has at most 16, 32, 64 members.  grid: (bundles, nchunk[, d]);
// part: [product][nchunk][T][64], entry (i, j) of a group in its member i's row at column j
template <int MODE, int BT>
__global__ __launch_bounds__(256) void lgo_block_kernel(const double *__restrict__ A,
                                                        const double *__restrict__ P, int n,
                                                        int npad, int cw,
                                                        const int *__restrict__ idx,
                                                        const int *__restrict__ start,
                                                        const int *__restrict__ bundle, long T,
                                                        double *__restrict__ part)
{
    __shared__ double sa[BQ_LGO_SLAB * BQ_LGO_LD];
    __shared__ double sb[MODE == LGO_BP ? BQ_LGO_SLAB * BQ_LGO_LD : 1];
    __shared__ int gi[BQ_LGO_MAXB]; // the members' indices
    __shared__ int go[BQ_LGO_MAXB]; // where each member's group begins among the members
    __shared__ int lowest;
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
    const int g0 = bundle[blockIdx.x], g1 = bundle[blockIdx.x + 1];
    const int s0 = start[g0], b = start[g1] - s0;
    const int chunk = blockIdx.y, nchunk = gridDim.y;
    const int prod = MODE == LGO_BP ? 1 + (int)blockIdx.z : 0;
    if (MODE == LGO_BP)
        A += (long)blockIdx.z * npad * npad;
    if (t < BQ_LGO_MAXB)
        gi[t] = t < b ? idx[s0 + t] : 0;
    if (t < g1 - g0) {
        const int from = start[g0 + t] - s0, to = start[g0 + t + 1] - s0;
        for (int m = from; m < to; ++m)
            go[m] = from;
    }
    __syncthreads();
    if (t == 0) {
        int lo = gi[0];
        for (int i = 1; i < b; ++i)
            lo = min(lo, gi[i]);
        lowest = lo;
    }
    __syncthreads();
    const int c0 = chunk * cw, cend = min(c0 + cw, n);
    // (the columns left of every row's diagonal hold nothing of an upper triangular matrix)
    const int first = MODE == LGO_YY && lowest > c0
                          ? c0 + (lowest - c0) / BQ_LGO_SLAB * BQ_LGO_SLAB
                          : c0;
    const bool mine = ti < b && tj < b;
    double acc[BT][BT];
#pragma unroll
    for (int a = 0; a < BT; ++a)
#pragma unroll
        for (int c = 0; c < BT; ++c)
            acc[a][c] = 0.0;
    const double *right = MODE == LGO_BP ? sb : sa;
    for (int m0 = first; m0 < cend; m0 += BQ_LGO_SLAB) {
        if (MODE == LGO_PP)
            lgo_stage_cols(P, npad, gi, b, m0, cend, sa);
        else
            lgo_stage_rows(A, npad, gi, b, m0, cend, MODE == LGO_YY, sa);
        if (MODE == LGO_BP)
            lgo_stage_cols(P, npad, gi, b, m0, cend, sb);
        __syncthreads();
        if (mine) {
#pragma unroll 4
            for (int mm = 0; mm < BQ_LGO_SLAB; ++mm) {
                double av[BT], bv[BT];
#pragma unroll
                for (int a = 0; a < BT; ++a)
                    av[a] = sa[mm * BQ_LGO_LD + ti + 16 * a];
#pragma unroll
                for (int c = 0; c < BT; ++c)
                    bv[c] = right[mm * BQ_LGO_LD + tj + 16 * c];
#pragma unroll
                for (int a = 0; a < BT; ++a)
#pragma unroll
                    for (int c = 0; c < BT; ++c)
                        acc[a][c] += av[a] * bv[c];
            }
        }
        __syncthreads();
    }
    if (!mine)
        return;
    double *out = part + (((long)prod * nchunk + chunk) * T + s0) * 64;
#pragma unroll
    for (int a = 0; a < BT; ++a)
#pragma unroll
        for (int c = 0; c < BT; ++c) {
            const int i = ti + 16 * a, j = tj + 16 * c;
            if (i < b && j < b && go[i] == go[j])
                out[(long)i * 64 + (j - go[j])] = acc[a][c];
        }
}

// entry (i, j) of a group's block of one product: the chunks' partials in their order
__device__ __forceinline__ double lgo_entry(const double *__restrict__ part, int prod, int nchunk,
                                            long T, long row, int j)
{
    double v = 0.0;
    for (int ch = 0; ch < nchunk; ++ch)
        v += part[(((long)prod * nchunk + ch) * T + row) * 64 + j];
    return v;
}

// Group blockIdx.x: sig (its b rows of 64: Sigma_B), r, mu, var (b each, at the group's place in
// the order of idx), lp and a_B.r_B (one each).  A pivot of P_BB that is not positive and finite
// sets *flag and ends the group.  grid: (G)
__global__ __launch_bounds__(256) void lgo_group_kernel(
    const double *__restrict__ part, int nchunk, long T, const int *__restrict__ idx,
    const int *__restrict__ start, const double *__restrict__ alpha, const double *__restrict__ y,
    double *__restrict__ sig, double *__restrict__ r, double *__restrict__ mu,
    double *__restrict__ var, double *__restrict__ lp, double *__restrict__ ar, int *flag)
{
    // P_BB, then its lower Cholesky factor, row-major; above the diagonal the transpose of
    // W = C^-1 (lower): W(m, j) at C[j * 64 + m], m > j, and its diagonal in wd
    __shared__ double C[64 * 64];
    __shared__ double av[64], zv[64], rv[64], wd[64];
    const int t = threadIdx.x;
    const int s0 = start[blockIdx.x], b = start[blockIdx.x + 1] - s0;
    for (int e = t; e < b * 64; e += 256) {
        const int i = e >> 6, j = e & 63;
        if (j <= i)
            C[e] = lgo_entry(part, 0, nchunk, T, s0 + i, j);
    }
    if (t < b)
        av[t] = alpha[idx[s0 + t]];
    __syncthreads();
    // right-looking Cholesky of the lower triangle
    for (int k = 0; k < b; ++k) {
        const double p = C[k * 64 + k];
        if (!(p > 0.0) || !(p <= 1.79769313486231570815e308)) { // (the same p in every thread)
            if (t == 0)
                *flag = 1;
            return;
        }
        const double c = sqrt(p);
        __syncthreads();
        if (t == 0)
            C[k * 64 + k] = c;
        else if (k + t < b)
            C[(k + t) * 64 + k] /= c;
        __syncthreads();
        const int m = b - k - 1;
        for (int e = t; e < m * m; e += 256) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i)
                C[i * 64 + j] -= C[i * 64 + k] * C[j * 64 + k];
        }
        __syncthreads();
    }
    // C z = a_B, C^T r = z: thread i keeps entry i
    double x = t < b ? av[t] : 0.0;
    for (int k = 0; k < b; ++k) {
        if (t == k)
            zv[k] = x / C[k * 64 + k];
        __syncthreads();
        if (t > k && t < b)
            x -= C[t * 64 + k] * zv[k];
    }
    x = t < b ? zv[t] : 0.0;
    for (int k = b - 1; k >= 0; --k) {
        if (t == k)
            rv[k] = x / C[k * 64 + k];
        __syncthreads();
        if (t < k)
            x -= C[k * 64 + t] * rv[k];
    }
    // W = C^-1: thread j solves C w = e_j down its own column
    if (t < b) {
        const int j = t;
        const double wjj = 1.0 / C[j * 64 + j];
        wd[j] = wjj;
        for (int i = j + 1; i < b; ++i) {
            double v = C[i * 64 + j] * wjj;
            for (int m = j + 1; m < i; ++m)
                v += C[i * 64 + m] * C[j * 64 + m];
            C[j * 64 + i] = -v / C[i * 64 + i];
        }
    }
    __syncthreads();
    // Sigma_B = W^T W
    for (int e = t; e < b * 64; e += 256) {
        const int i = e >> 6, j = e & 63;
        if (j < b) {
            const int lo = min(i, j), hi = max(i, j);
            // m = hi: W(hi, hi) W(hi, lo)
            double v = wd[hi] * (lo == hi ? wd[hi] : C[lo * 64 + hi]);
            for (int m = hi + 1; m < b; ++m)
                v += C[i * 64 + m] * C[j * 64 + m];
            sig[(long)(s0 + i) * 64 + j] = v;
            if (i == j)
                var[s0 + i] = v;
        }
    }
    if (t < b) {
        r[s0 + t] = rv[t];
        mu[s0 + t] = y[idx[s0 + t]] - rv[t];
    }
    if (t == 0) {
        double ld = 0.0, q = 0.0; // 1/2 log|P_BB| = sum log C_kk
        for (int k = 0; k < b; ++k) {
            ld += log(C[k * 64 + k]);
            q += av[k] * rv[k];
        }
        ar[blockIdx.x] = q;
        lp[blockIdx.x] = ld - 0.5 * q - b * BQ_HALF_LOG_2PI;
    }
}

// Group blockIdx.x: its d + 2 entries of dL_lgo / dtheta over [h, w_1 .. w_d, s] into
// gpart[group][d + 2].  part: Q_BB (product 0) and M_1 .. M_d; Z: the d + 2 vectors P (D_p a),
// npad apart.  grid: (G)
__global__ __launch_bounds__(256) void lgo_group_grad_kernel(
    const double *__restrict__ part, int nchunk, long T, const int *__restrict__ idx,
    const int *__restrict__ start, const double *__restrict__ sig, const double *__restrict__ r,
    const double *__restrict__ ar, const double *__restrict__ Z, int d, int npad, double h,
    double s, double s2, double *__restrict__ gpart)
{
    __shared__ double red[256];
    __shared__ double rv[64];
    __shared__ double rXr[BQ_MAXD + 1], trSX[BQ_MAXD + 1], rZ[BQ_MAXD + 2];
    const int t = threadIdx.x;
    const int s0 = start[blockIdx.x], b = start[blockIdx.x + 1] - s0;
    if (t < b)
        rv[t] = r[s0 + t];
    __syncthreads();
    for (int z = 0; z <= d; ++z) {
        double v1 = 0.0, v2 = 0.0;
        for (int e = t; e < b * 64; e += 256) {
            const int i = e >> 6, j = e & 63;
            if (j < b) {
                const double xv = lgo_entry(part, z, nchunk, T, s0 + i, j);
                v1 += rv[i] * xv * rv[j];
                v2 += sig[(long)(s0 + i) * 64 + j] * xv; // (Sigma_B is symmetric)
            }
        }
        v1 = wg_tree_sum(v1, red);
        v2 = wg_tree_sum(v2, red);
        if (t == 0) {
            rXr[z] = v1;
            trSX[z] = v2;
        }
    }
    for (int p = 0; p < d + 2; ++p) {
        double v = t < b ? rv[t] * Z[(long)p * npad + idx[s0 + t]] : 0.0;
        v = wg_tree_sum(v, red);
        if (t == 0)
            rZ[p] = v;
    }
    if (t == 0) {
        double *g = gpart + (long)blockIdx.x * (d + 2);
        // r^T M_h r = (2 / h)(a_B.r_B - s^2 r^T Q r), tr(Sigma_B M_h) = (2 / h)(b - s^2 tr(Sigma_B Q))
        g[0] = rZ[0] - ((ar[blockIdx.x] - s2 * rXr[0]) + ((double)b - s2 * trSX[0])) / h;
        for (int k = 1; k <= d; ++k)
            g[k] = rZ[k] - 0.5 * (rXr[k] + trSX[k]);
        g[d + 1] = rZ[d + 1] - s * (rXr[0] + trSX[0]);
    }
}
