// remove.h -- shrinking a resident GP fit by k observations without refactoring it (fit.hip,
// bq_gp_remove): the compaction into a layout of n - k points and the rank-k update of the
// compacted factor.  Part of the libbqhip.so kernel set; compiled into k_reduce.hip (host.h lists
// the units).
//
// With R the removed indices and keep the rest, A[keep, keep] = Lc Lc^T + V V^T, Lc = L[keep, keep]
// (still lower triangular), V = L[keep, R] (zero wherever keep[i] < R[j]).  The factor of the
// survivors is the L' of [Lc V] Q = [L' 0] with Q orthogonal, built one 64-column block J at a
// time from 64 columns of V: with L11, V1 the block's diagonal tile and its rows of V,
//   L11' = chol(L11 L11^T + V1 V1^T),  W = L11^-1 V1,  C C^T = I + W^T W,
//   M = [[L11^T L11'^-T, -W C^-T], [V1^T L11'^-T, C^-T]]     (128 x 128, orthogonal)
// and every row block below takes [L21' V2'] = [L21 V2] M -- the block formulas
//   L21' = (L21 L11^T + V2 V1^T) L11'^-T,  V2' = (V2 - L21 W) C^-T
// as one 128-deep product.  z = L^-1 y is a row of the same system ([z_keep^T z_R^T] in the border
// block) and transforms with the rows: no solve of its own.  A positive-semidefinite matrix is
// added, no pivot can cancel: there is no "not positive definite" outcome.
// Two launches per block column: remove_diag_kernel (one workgroup: L11' in place, M into scratch)
// and remove_rows_kernel (a workgroup per 64-row block below, MFMA).  No atomics, every sum has a
// fixed order: the same bits from run to run.
#pragma once
#include "common.h"
#include "wgsum.h"

#define BQ_REMOVE_LD 65                              // leading dimension of the LDS tiles
#define BQ_REMOVE_TILE (64 * BQ_REMOVE_LD)
#define BQ_REMOVE_LDS_DOUBLES (4 * BQ_REMOVE_TILE + 2 * 64) // L11 | V1 | G, H | W, two diagonals
// (BQ_REMOVE_M_DOUBLES, struct RemoveJob: types.h; M(k, c) at M[c + 128 k])

// One pass from the old fit into buffers of the new layout: the survivors' rows and columns of the
// factor with the identity on the padding, the border block (z of the survivors in the y row, the
// identity beside it as the assembly leaves it), V with z of the removed in its y row, the
// survivors' points and targets.  Tiles strictly above the diagonal are not written (nothing reads
// them).  grid (ntot2 / 64, npad2 / 64 + 1 + kp / 64), 256 threads: a 64 x 64 tile each.
__global__ __launch_bounds__(256) void remove_compact_kernel(RemoveJob r)
{
    const int t = threadIdx.x, li = t & 63, lj0 = t >> 6;
    const int bi = blockIdx.x, bj = blockIdx.y, nbl = r.npad2 / 64;
    const int i2 = 64 * bi + li;
    const bool isz = i2 == r.npad2; // (the new layout has no border points: its y row)
    long src = 0;                   // this row in the old system
    if (i2 < r.n2)
        src = r.keep[i2];
    else if (isz)
        src = r.yrow;
    if (bj == 0 && t < 64) {
        if (i2 < r.npad2)
            r.y2[i2] = i2 < r.n2 ? r.y[src] : 0.0;
        for (int m = 0; m < r.d; ++m)
            r.pts2[(long)i2 * r.d + m] = i2 < r.n2 ? r.pts[src * r.d + m] : 0.0;
    }
    if (bj < nbl) {
        if (bj > bi)
            return;
        for (int c = 0; c < 16; ++c) {
            const int j2 = 64 * bj + lj0 + 4 * c;
            double v;
            if (i2 >= r.npad2)
                v = (isz && j2 < r.n2) ? r.A[src + (long)r.keep[j2] * r.ldl] : 0.0;
            else if (i2 < r.n2 && j2 < r.n2)
                v = j2 <= i2 ? r.A[src + (long)r.keep[j2] * r.ldl] : 0.0;
            else
                v = i2 == j2 ? 1.0 : 0.0;
            r.A2[i2 + (long)j2 * r.ldl2] = v;
        }
    } else if (bj == nbl) {
        if (bi != nbl)
            return;
        for (int c = 0; c < 16; ++c) {
            const int j2 = r.npad2 + lj0 + 4 * c;
            r.A2[i2 + (long)j2 * r.ldl2] = (i2 == j2 && !isz) ? 1.0 : 0.0;
        }
    } else {
        for (int c = 0; c < 16; ++c) {
            const int jv = 64 * (bj - nbl - 1) + lj0 + 4 * c;
            double v = 0.0;
            if (jv < r.k) {
                const long rj = r.rem[jv];
                if (isz || (i2 < r.n2 && src > rj))
                    v = r.A[src + rj * r.ldl];
            }
            r.V[i2 + (long)jv * r.ntot2] = v;
        }
    }
}

// The removed observations are exactly the last ones and the layout stays: rows [n2, n) of the
// factor become the identity again, their entries of the y row, the points and the targets are
// cleared.  grid ceil(npad / 256), 256 threads: a column each.
__global__ __launch_bounds__(256) void remove_trail_kernel(double *__restrict__ A, long ldl,
                                                           int yrow, double *__restrict__ pts,
                                                           double *__restrict__ y, int d, int n2,
                                                           int n, int npad)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= npad)
        return;
    for (int i = n2; i < n; ++i)
        A[i + (long)j * ldl] = i == j ? 1.0 : 0.0;
    if (j >= n2 && j < n) {
        A[yrow + (long)j * ldl] = 0.0;
        y[j] = 0.0;
        for (int m = 0; m < d; ++m)
            pts[(long)j * d + m] = 0.0;
    }
}

// acc += X(i0 + ., :) X(j0 + ., :)^T over nk columns on v_mfma_f64_16x16x4_f64; X(i, k) at
// X[i rs + k ks].  Register r of the result is entry (i0 + l4 + 4 r, j0 + l15).
__device__ __forceinline__ double4_t remove_xxt(const double *X, int rs, int ks, int nk, int i0,
                                                int j0, int l15, int l4, double4_t acc)
{
    for (int k0 = 0; k0 < nk; k0 += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[(i0 + l15) * rs + (k0 + l4) * ks],
                                                   X[(j0 + l15) * rs + (k0 + l4) * ks], acc, 0, 0, 0);
    return acc;
}

// In-place lower Cholesky factor of the 64 x 64 tile S (LDS, ld BQ_REMOVE_LD), right-looking, the
// reciprocal diagonal into rd.  The pivots stay squared in place until the end: two barriers per
// column.  Ends with a barrier.  256 threads.
__device__ __forceinline__ void remove_chol64(double *S, double *rd, int t)
{
    for (int j = 0; j < 64; ++j) {
        const double ljj = sqrt(S[BQ_REMOVE_LD * j + j]);
        if (t > j && t < 64)
            S[BQ_REMOVE_LD * t + j] = S[BQ_REMOVE_LD * t + j] / ljj;
        __syncthreads();
        const int i = j + 1 + (t & 63);
        if (i < 64) {
            const double lij = S[BQ_REMOVE_LD * i + j];
            for (int cc = j + 1 + (t >> 6); cc <= i; cc += 4)
                S[BQ_REMOVE_LD * i + cc] =
                    fma(-lij, S[BQ_REMOVE_LD * cc + j], S[BQ_REMOVE_LD * i + cc]);
        }
        __syncthreads();
    }
    if (t < 64) {
        const double l = sqrt(S[BQ_REMOVE_LD * t + t]);
        S[BQ_REMOVE_LD * t + t] = l;
        rd[t] = 1.0 / l;
    }
    __syncthreads();
}

// x <- L^-1 x for one column held in registers; L (LDS, ld BQ_REMOVE_LD) and its reciprocal
// diagonal are read as broadcasts.
__device__ __forceinline__ void remove_solve_col(const double *L, const double *rd, double (&x)[64])
{
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const double xk = x[k] * rd[k];
        x[k] = xk;
#pragma unroll
        for (int i = k + 1; i < 64; ++i)
            x[i] = fma(-L[BQ_REMOVE_LD * i + k], xk, x[i]);
    }
}

// Block column J of the update, one workgroup of 256 threads, BQ_REMOVE_LDS_DOUBLES of dynamic
// LDS: the diagonal tile of A (ld lda, lower) becomes L11' in place, and M (header) goes into Ms
// for remove_rows_kernel.  V: this sweep's 64 columns (ld ldv).
__global__ __launch_bounds__(256) void remove_diag_kernel(double *__restrict__ A, long lda,
                                                          const double *__restrict__ V, long ldv,
                                                          int J, double *__restrict__ Ms)
{
    extern __shared__ __attribute__((aligned(16))) double remove_lds[];
    double *a = remove_lds, *b = a + BQ_REMOVE_TILE, *g = b + BQ_REMOVE_TILE,
           *e = g + BQ_REMOVE_TILE, *rda = e + BQ_REMOVE_TILE, *rdg = rda + 64;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, l15 = lane & 15, l4 = lane >> 4;
    double *Ad = A + 64L * J + 64L * J * lda;
    const double *Vd = V + 64L * J;
    for (int c = 0; c < 16; ++c) {
        const int j = w + 4 * c;
        a[BQ_REMOVE_LD * lane + j] = j <= lane ? Ad[lane + (long)j * lda] : 0.0;
        b[BQ_REMOVE_LD * lane + j] = Vd[lane + (long)j * ldv];
    }
    __syncthreads();
    if (t < 64)
        rda[t] = 1.0 / a[BQ_REMOVE_LD * t + t];
    // G = L11 L11^T + V1 V1^T: wave w the tiles (w, 0 .. w)
    for (int tj = 0; tj <= w; ++tj) {
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
        acc = remove_xxt(a, BQ_REMOVE_LD, 1, 64, 16 * w, 16 * tj, l15, l4, acc);
        acc = remove_xxt(b, BQ_REMOVE_LD, 1, 64, 16 * w, 16 * tj, l15, l4, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            g[BQ_REMOVE_LD * (16 * w + l4 + 4 * r) + 16 * tj + l15] = acc[r];
    }
    __syncthreads();
    remove_chol64(g, rdg, t);
    for (int c = 0; c < 16; ++c) {
        const int j = w + 4 * c;
        if (j <= lane)
            Ad[lane + (long)j * lda] = g[BQ_REMOVE_LD * lane + j];
    }
    // columns 0 .. 127 of M^T's left half: L11'^-1 [L11 V1] (waves 0, 1); W = L11^-1 V1 (wave 2)
    if (w < 3) {
        const double *src = w == 0 ? a + lane : b + lane;
        const double *Lm = w < 2 ? g : a, *rd = w < 2 ? rdg : rda;
        double x[64];
#pragma unroll
        for (int i = 0; i < 64; ++i)
            x[i] = src[BQ_REMOVE_LD * i];
        remove_solve_col(Lm, rd, x);
        if (w < 2) {
#pragma unroll
            for (int i = 0; i < 64; ++i)
                Ms[i + 128 * t] = x[i];
        } else {
#pragma unroll
            for (int i = 0; i < 64; ++i)
                e[BQ_REMOVE_LD * i + lane] = x[i];
        }
    }
    __syncthreads();
    // H = I + W^T W over G, then C = chol(H)
    for (int tj = 0; tj <= w; ++tj) {
        double4_t acc;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[r] = (16 * w + l4 + 4 * r == 16 * tj + l15) ? 1.0 : 0.0;
        acc = remove_xxt(e, 1, BQ_REMOVE_LD, 64, 16 * w, 16 * tj, l15, l4, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            g[BQ_REMOVE_LD * (16 * w + l4 + 4 * r) + 16 * tj + l15] = acc[r];
    }
    __syncthreads();
    remove_chol64(g, rdg, t);
    // M's right half, as columns of its transpose: C^-1 (-W^T) (wave 1), C^-1 (wave 0)
    if (w < 2) {
        double x[64];
#pragma unroll
        for (int i = 0; i < 64; ++i)
            x[i] = w == 0 ? (i == lane ? 1.0 : 0.0) : -e[BQ_REMOVE_LD * lane + i];
        remove_solve_col(g, rdg, x);
        double *out = Ms + 64 + 128 * (w == 0 ? 64 + lane : lane);
#pragma unroll
        for (int i = 0; i < 64; ++i)
            out[i] = x[i];
    }
}

// [L21' V2'] = [L21 V2] M for the row blocks below block column J: grid (row blocks below J, the
// border block included), 256 threads, wave w the rows 16 w .. 16 w + 15 of its block.  Issued as
// D^T = M^T X^T so that 16 lanes cover 16 consecutive rows of a column (whole 128-byte lines).  A
// wave reads all of its rows before it writes any of them and no other wave touches them: in place.
__global__ __launch_bounds__(256) void remove_rows_kernel(double *__restrict__ A, long lda,
                                                          double *__restrict__ V, long ldv, int J,
                                                          const double *__restrict__ Ms)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const long row = 64L * (J + 1 + blockIdx.x) + 16 * w + l15;
    double *Ar = A + row + 64L * J * lda, *Vr = V + row;
    const double *Mr = Ms + l15;
    double4_t acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c)
        acc[c] = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int k0 = 0; k0 < 64; k0 += 4) {
        const double x = Ar[(long)(k0 + l4) * lda];
#pragma unroll
        for (int c = 0; c < 8; ++c)
            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(Mr[16 * c + 128 * (k0 + l4)], x, acc[c], 0,
                                                         0, 0);
    }
#pragma unroll 4
    for (int k0 = 0; k0 < 64; k0 += 4) {
        const double x = Vr[(long)(k0 + l4) * ldv];
#pragma unroll
        for (int c = 0; c < 8; ++c)
            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(Mr[16 * c + 128 * (64 + k0 + l4)], x,
                                                         acc[c], 0, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Ar[(long)(16 * c + l4 + 4 * r) * lda] = acc[c][r];
            Vr[(long)(16 * c + l4 + 4 * r) * ldv] = acc[4 + c][r];
        }
}

// The scalars of the shrunk fit, one workgroup: logdet = 2 sum log L_ii and qf = |z|^2 over the n
// survivors in a fixed order, logml = -qf/2 - logdet/2 - n/2 log 2 pi; the reciprocal diagonal.
// out: the words a (re)fit reads back, [info = 0 | - | logml, logdet, qf].
__global__ __launch_bounds__(256) void remove_finish_kernel(const double *__restrict__ A, long lda,
                                                            int yrow, int n, int npad,
                                                            double *__restrict__ dinv,
                                                            double *__restrict__ out)
{
    __shared__ double pl[256], pq[256];
    const int t = threadIdx.x;
    double sl = 0.0, sq = 0.0;
    for (int i = t; i < npad; i += 256) {
        const double l = A[i + (long)i * lda];
        dinv[i] = 1.0 / l;
        if (i < n) {
            sl += log(l);
            const double z = A[yrow + (long)i * lda];
            sq = fma(z, z, sq);
        }
    }
    wg_tree_add2(sl, sq, pl, pq);
    if (t == 0) {
        reinterpret_cast<int *>(out)[0] = 0;
        const double logdet = 2.0 * pl[0], qf = pq[0];
        out[2] = -0.5 * qf - 0.5 * logdet - 0.5 * (double)n * 1.8378770664093453;
        out[3] = logdet;
        out[4] = qf;
    }
}
