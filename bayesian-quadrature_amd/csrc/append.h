// append.h -- growing a resident GP fit by k observations without refactoring it (fit.hip,
// bq_gp_append): the Schur complement of the new points, its factor and the stores into the fit.
// Part of the libbqhip.so kernel set; compiled into k_reduce.hip (host.h lists the units).
//
// With V = K(x_new, x_old) L^-T (the 64-column row sweep, k rows padded to kp) the new factor is
// [[L, 0], [V, L_S]], L_S L_S^T = S = K(x_new, x_new) + s^2 I - V V^T, and the new part of
// z = L^-1 y is z_new = L_S^-1 (y_new - V z).  Everything is computed in side buffers; only
// append_commit_kernel writes into the fit, and only when every pivot was positive.  No atomics:
// every sum has a fixed order, the results are the same bits from run to run.
#pragma once
#include "common.h"
#include "wgsum.h"

#define BQ_APPEND_CHUNK 256                  // columns of V per workgroup of append_part_kernel
#define BQ_APPEND_PART (64 * 64 + 64)        // doubles per workgroup: V V^T (ld 64), then V z

// (struct AppendJob: types.h)

// Partial sums of V V^T (lower 4 x 4 micro-tiles, rows < k) and of V z over one chunk of
// BQ_APPEND_CHUNK columns per workgroup; k <= 64, V has 64 rows (ld 64).  z is row `yrow` of the
// factor (stride ldl).  grid: ceil(npad / BQ_APPEND_CHUNK), 256 threads.
__global__ __launch_bounds__(256) void append_part_kernel(const double *__restrict__ V, int npad,
                                                          int k, const double *__restrict__ z,
                                                          long zstride, double *__restrict__ part)
{
    __shared__ double sV[64][65]; // [column][row]
    __shared__ double sz[64];
    const int t = threadIdx.x, ti = t & 15, tj = t >> 4;
    const int c0 = blockIdx.x * BQ_APPEND_CHUNK;
    const int c1 = min(c0 + BQ_APPEND_CHUNK, npad);
    const bool mine = tj <= ti && 4 * ti < k; // (then 4 tj < k as well)
    double acc[4][4] = {{0.0}};
    double vz = 0.0;
    for (int cb = c0; cb < c1; cb += 64) { // npad is a multiple of 64
        for (int e = t; e < 64 * 64; e += 256) {
            const int r = e & 63, cc = e >> 6;
            sV[cc][r] = V[r + (long)(cb + cc) * 64];
        }
        if (t < 64)
            sz[t] = z[(long)(cb + t) * zstride];
        __syncthreads();
        if (mine) {
            for (int cc = 0; cc < 64; ++cc) {
                double a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a[u] = sV[cc][4 * ti + u];
                    b[u] = sV[cc][4 * tj + u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        acc[u][v] = fma(a[u], b[v], acc[u][v]);
            }
        }
        if (t < 64)
            for (int cc = 0; cc < 64; ++cc)
                vz = fma(sV[cc][t], sz[cc], vz);
        __syncthreads();
    }
    double *p = part + (long)blockIdx.x * BQ_APPEND_PART;
    if (mine) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                p[(4 * ti + u) + 64 * (4 * tj + v)] = acc[u][v];
    }
    if (t < 64)
        p[64 * 64 + t] = vz;
}

// k(p, q) with the arithmetic of gauss_q / exp_gauss for a run-time dimension
__device__ __forceinline__ double append_kernel_value(const double *p, const double *q, int d,
                                                      const GaussParams &g)
{
    double acc = 0.0;
    for (int m = 0; m < d; ++m) {
        const double t = p[m] - q[m];
        acc += (t * t) * g.nh[m];
    }
    return g.c * exp_gauss(acc);
}

// One workgroup, k <= 64: sums the partials in their order, S = K(x_new, x_new) + s^2 I - V V^T,
// factors it (right-looking, in LDS) and solves L_S z_new = y_new - V z.  Writes L_S into the lower
// triangle of S (ld 64) with the identity on the padding, z_new into zn[0 .. 64), and into info the
// 1-based index of the first pivot that is not above tol and finite (0: none).
// tol (fit.hip, append_pivot_tol): a pivot is a difference of numbers of the size of the kernel's
// diagonal, and the factor it completes is the exact factor of a matrix within 4 (n + k + 1) eps
// of that size per entry (Higham, Accuracy and Stability, thm 10.3) -- a pivot no larger than
// that says a matrix within the factorisation's own rounding error is singular: an exact duplicate
// of an old point at s = 0 leaves +-1e-16 of the diagonal there, of either sign.
__global__ __launch_bounds__(256) void append_factor_kernel(const double *__restrict__ part,
                                                            int nparts,
                                                            const double *__restrict__ xn,
                                                            const double *__restrict__ yn, int d,
                                                            int k, GaussParams g, double tol,
                                                            double *__restrict__ S,
                                                            double *__restrict__ zn,
                                                            int *__restrict__ info)
{
    __shared__ double sS[64][65]; // [row][column]
    __shared__ double sr[64];
    __shared__ int bad;
    const int t = threadIdx.x;
    if (t == 0)
        bad = 0;
    for (int e = t; e < 64 * 64; e += 256) {
        const int i = e & 63, j = e >> 6;
        double v = (i == j) ? 1.0 : 0.0;
        if (j <= i && i < k) {
            double s = 0.0;
            for (int p = 0; p < nparts; ++p)
                s += part[(long)p * BQ_APPEND_PART + i + 64 * j];
            v = append_kernel_value(xn + (long)i * d, xn + (long)j * d, d, g);
            if (i == j)
                v += g.s2;
            v -= s;
        }
        sS[i][j] = v;
    }
    if (t < 64) {
        double r = 0.0;
        if (t < k) {
            double s = 0.0;
            for (int p = 0; p < nparts; ++p)
                s += part[(long)p * BQ_APPEND_PART + 64 * 64 + t];
            r = yn[t] - s;
        }
        sr[t] = r;
    }
    __syncthreads();
    for (int j = 0; j < k; ++j) {
        const double piv = sS[j][j];
        if (!(piv > tol) || !(piv < 1.79769313486231570815e308)) {
            if (t == 0)
                bad = j + 1;
            break; // (every thread reads the same pivot: the exit is uniform)
        }
        const double ljj = sqrt(piv);
        __syncthreads(); // every thread has read the pivot
        if (t == 0)
            sS[j][j] = ljj;
        for (int i = j + 1 + t; i < k; i += 256)
            sS[i][j] = sS[i][j] / ljj;
        __syncthreads();
        // trailing update of the lower triangle: (i, c), j < c <= i < k
        const int m = k - j - 1;
        for (int e = t; e < m * m; e += 256) {
            const int i = j + 1 + e % m, cc = j + 1 + e / m;
            if (cc <= i)
                sS[i][cc] = fma(-sS[i][j], sS[cc][j], sS[i][cc]);
        }
        __syncthreads();
    }
    __syncthreads();
    if (bad == 0) {
        // forward substitution, one unknown per step
        for (int j = 0; j < k; ++j) {
            if (t == j)
                sr[j] = sr[j] / sS[j][j];
            __syncthreads();
            if (t > j && t < k)
                sr[t] = fma(-sS[t][j], sr[j], sr[t]);
            __syncthreads();
        }
    }
    for (int e = t; e < 64 * 64; e += 256) {
        const int i = e & 63, j = e >> 6;
        if (j <= i)
            S[i + 64 * j] = sS[i][j];
    }
    if (t < 64)
        zn[t] = sr[t];
    if (t == 0)
        info[0] = bad;
}

// A block append (k > 64) after the device Cholesky of S, one workgroup: row 0 of X (64 x kp,
// ld 64, cleared by the caller) = y_new - V z, the right-hand side of the last solve; and the
// pivots L_S[j, j]^2 against tol as append_factor_kernel tests its own -- the first one at or below
// it goes into info (1-based) unless the factorisation has flagged a column already.
__global__ __launch_bounds__(256) void append_rhs_kernel(const double *__restrict__ yn,
                                                         const double *__restrict__ vz, int k,
                                                         double *__restrict__ X,
                                                         const double *__restrict__ S, int kp,
                                                         double tol, int *__restrict__ info)
{
    __shared__ int first[256];
    const int t = threadIdx.x;
    int mine = 0x7fffffff;
    for (int i = t; i < k; i += 256) {
        X[(long)i * 64] = yn[i] - vz[i];
        const double l = S[i + (long)i * kp];
        if (!(l * l > tol) && i < mine)
            mine = i;
    }
    // (wgsum.h's tree in its min form, written out: through wg_tree this kernel compiles to other code)
    first[t] = mine;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off)
            first[t] = min(first[t], first[t + off]);
        __syncthreads();
    }
    if (t == 0 && info[0] == 0 && first[0] != 0x7fffffff)
        info[0] = first[0] + 1;
}

// The only kernel that writes into the fit.  info != 0: nothing but the flag goes out.  Otherwise
// rows n .. n + k of the factor (V over the old points' columns, L_S behind them), z_new in the y
// row, the reciprocal diagonal, the points and the targets; workgroup 0 also writes the scalars,
//   logdet += 2 sum log diag L_S,  qf += |z_new|^2,  logml = -qf/2 - logdet/2 - (n + k)/2 log 2 pi.
// grid: any number of workgroups of 256 threads.
__global__ __launch_bounds__(256) void append_commit_kernel(AppendJob a)
{
    const int t = threadIdx.x;
    const int bad = a.info[0];
    if (blockIdx.x == 0) {
        __shared__ double pl[256], pq[256];
        double sl = 0.0, sq = 0.0;
        if (bad == 0)
            for (int i = t; i < a.k; i += 256) {
                sl += log(a.S[i + (long)i * a.kp]);
                const double z = a.zn[(long)i * a.zstride];
                sq = fma(z, z, sq);
            }
        wg_tree_add2(sl, sq, pl, pq);
        if (t == 0) {
            reinterpret_cast<int *>(a.out)[0] = bad;
            const double logdet = a.logdet + 2.0 * pl[0], qf = a.qf + pq[0];
            a.out[2] = -0.5 * qf - 0.5 * logdet - 0.5 * (double)(a.n + a.k) * 1.8378770664093453;
            a.out[3] = logdet;
            a.out[4] = qf;
        }
    }
    if (bad != 0)
        return;
    const long nthreads = (long)gridDim.x * 256, g0 = (long)blockIdx.x * 256 + t;
    // V: row i of the k new ones fastest (contiguous in V and in the factor)
    for (long e = g0; e < (long)a.k * a.n; e += nthreads) {
        const int i = (int)(e % a.k);
        const long c = e / a.k;
        a.A[a.n + i + c * a.ldl] = a.V[i + c * a.kp];
    }
    for (long e = g0; e < (long)a.k * a.k; e += nthreads) {
        const int i = (int)(e % a.k), j = (int)(e / a.k);
        if (j <= i)
            a.A[a.n + i + (long)(a.n + j) * a.ldl] = a.S[i + (long)j * a.kp];
    }
    for (long i = g0; i < a.k; i += nthreads) {
        a.A[a.yrow + (a.n + i) * a.ldl] = a.zn[i * a.zstride];
        a.dinv[a.n + i] = 1.0 / a.S[i + i * a.kp];
        a.y[a.n + i] = a.yn[i];
    }
    for (long e = g0; e < (long)a.k * a.d; e += nthreads)
        a.pts[(long)a.n * a.d + e] = a.xn[e];
}

// The border strip of a grown fit: rows [r0, ntot) of the new ntot x ntot system over all its
// columns -- zero, the identity on the padding's diagonal, and the old fit's z (row yold of Aold,
// its first ncopy columns) in the new y row, whose own diagonal entry is zero as the assembly
// leaves it.  grid (ceil((ntot - r0) / 256), ntot).
__global__ void append_grow_kernel(double *__restrict__ A, long lda, int r0, int ntot, int yrow,
                                   const double *__restrict__ Aold, long ldold, int yold, int ncopy)
{
    const int i = r0 + blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= ntot)
        return;
    double v = (i == j && i != yrow) ? 1.0 : 0.0;
    if (i == yrow && j < ncopy)
        v = Aold[yold + (long)j * ldold];
    A[i + (long)j * lda] = v;
}
