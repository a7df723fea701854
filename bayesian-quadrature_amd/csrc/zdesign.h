// zdesign.h -- the integral Z = int f(x) N(x | mu, Sigma) dx of a resident fit and the greedy
// design that lowers its posterior variance the most: sequential Bayesian quadrature (fit.hip,
// bq_gp_integral and bq_gp_zdesign; include/bqhip.h has the contracts).
// Part of the libbqhip.so kernel set; compiled into k_reduce.hip (host.h lists the units).
//
// A candidates may be observed.  With dc = diag Sigma(xc, xc) and u_a = Cov(Z, f(xc_a) | data) =
// kappa(xc_a) - v_a . b (b = L^-1 kappa_X, the fit's KMEAN state), step t is
//     score[a] = u_a^2 / (dc[a] + nugget)                         the drop of var Z
//     p        = the first largest score among the eligible candidates
//     den      = sqrt(dc[p] + nugget)
//     c        = (K(xc, xc_p) - W[:, :npad + t] W[p, :npad + t]^T) / den
//     u       -= c (u_p / den),  dc -= c o c.
// W = [V | C] is the prediction's workspace with the earlier c behind V, as in pivchol.h, whose
// pivchol_col_kernel forms the product.  No reference points and no A x R matrix: a step reads W
// once and a few vectors.  Three launches a step, none of which waits for the host: the pivot, its
// score and the done flag live in a PivcholState on the device, dc[p] + nugget and u_p in two
// doubles beside it.
//   zd_vb_kernel         once: V b in slices, pivchol_col_kernel's pass with b for the pivot's row
//   zd_start_kernel      dc, u, no row taken, step 0's scores, each workgroup's first candidate
//   pivchol_col_kernel   (pivchol.h) the row-gathered product over the candidate rows of W
//   zd_finish_kernel     the slices summed in order, the kernel value, the division, c into
//                        column npad + t of W, dc, u, step t + 1's scores on the way and each
//                        workgroup's first candidate
//   zd_pick_kernel       one workgroup: the argmax, the stop rule, piv[t], gain[t], dc[p] + nugget,
//                        u_p, the done flag
// After the done flag every kernel returns at once.
//
// Determinism: the product over W is pivchol's (KS from pivchol_plan, the slices added in ascending
// order), everything else is one thread per candidate: a step's bits depend on the shapes and on
// t, never on q.  No floating-point atomics.
#pragma once
#include "pivchol.h"

// *out = sum_j a[j] b[j] over n entries: thread t takes j = t, t + 256, .. in ascending order,
// then a fixed tree.  One workgroup of 256 threads.  (b.b and b.z of bq_gp_integral.)
__global__ __launch_bounds__(256) void zd_dot_kernel(const double *__restrict__ a,
                                                     const double *__restrict__ b, int n,
                                                     double *__restrict__ out)
{
    __shared__ double sv[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int j = t; j < n; j += 256)
        s = __builtin_fma(a[j], b[j], s);
    sv[t] = s;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h)
            sv[t] += sv[t + h];
        __syncthreads();
    }
    if (t == 0)
        *out = sv[0];
}

// a candidate's score and whether it is eligible: dc + nugget > 0 and, with nugget = 0, not taken
__device__ __forceinline__ bool zd_score(double u, double dc, double nugget, int taken, double *sc)
{
    const double den2 = dc + nugget;
    const bool ok = den2 > 0.0 && !(nugget == 0.0 && taken);
    *sc = ok ? u * u / den2 : 0.0;
    return ok;
}

// part[slice y][row] = sum over k in the slice of V[row, k] b[k], K = npad columns in slices of
// KS <= BQ_PIVCHOL_KS_MAX: pivchol_col_kernel's pass over V -- grid (Ap / RB, ceil(K / KS)), RB
// threads, one row each, BQ_PIVCHOL_U loads in flight and as many accumulators that take their k
// in ascending order and are folded in a fixed tree -- with the slice's piece of the contiguous b
// in LDS where that kernel gathers row p of W.  (rowdot_kernel with b for z gives the same sums,
// but in 16-row workgroups whose waves read 128 bytes of a column: the LABBOOK has both rates.)
template <int RB>
__global__ __launch_bounds__(RB) void zd_vb_kernel(const double *__restrict__ V, long ld, int K,
                                                   int KS, const double *__restrict__ b,
                                                   double *__restrict__ part)
{
    constexpr int U = BQ_PIVCHOL_U;
    __shared__ double u[BQ_PIVCHOL_KS_MAX];
    const int t = threadIdx.x;
    const long row = (long)blockIdx.x * RB + t;
    const int k0 = (int)blockIdx.y * KS, len = min(KS, K - k0);
    for (int k = t; k < len; k += RB)
        u[k] = b[k0 + k];
    __syncthreads();
    const double *w = V + row + (long)k0 * ld;
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

// dc = var (bq_gp_predict's variance bits) and u = kap - V b (zd_vb_kernel's nsl slices, ld apart,
// summed in order) on the A candidates, 0 on the padding of either; no row taken; step 0's scores
// into score0 (0 where not eligible) and each workgroup's first candidate; workgroup 0: piv = -1,
// gain = 0, the state with rank = q.  grid ceil(Ap / 256).
__global__ __launch_bounds__(256) void zd_start_kernel(
    const double *__restrict__ var, const double *__restrict__ kap,
    const double *__restrict__ part, long ld, int nsl,
    int A, int Ap, int q, double nugget, PivcholState *st, double *__restrict__ den2,
    long long *__restrict__ piv, double *__restrict__ gain, double *__restrict__ dc,
    double *__restrict__ u, int *__restrict__ taken, double *__restrict__ score0,
    double *__restrict__ candv, int *__restrict__ candi)
{
    __shared__ double sv[256];
    __shared__ int si[256];
    const int t = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + t;
    double v = -INFINITY;
    int idx = INT_MAX;
    if (i < Ap) {
        const double di = i < A ? var[i] : 0.0;
        double ui = 0.0;
        if (i < A) {
            double s = 0.0;
            for (int y = 0; y < nsl; ++y)
                s += part[(long)y * ld + i];
            ui = kap[i] - s;
        }
        dc[i] = di, u[i] = ui;
        taken[i] = 0;
        double sc = 0.0;
        if (i < A && zd_score(ui, di, nugget, 0, &sc))
            v = sc, idx = (int)i;
        score0[i] = sc;
    }
    if (blockIdx.x == 0) {
        for (int k = t; k < q; k += 256)
            piv[k] = -1, gain[k] = 0.0;
        if (t == 0) {
            st->done = 0, st->rank = q, st->p = 0, st->pad = 0, st->gain = 0.0;
            den2[0] = 1.0, den2[1] = 0.0;
        }
    }
    pivchol_wg_first(v, idx, sv, si);
    if (t == 0)
        candv[blockIdx.x] = sv[0], candi[blockIdx.x] = si[0];
}

// Step t's pivot out of the nblk candidates (pivchol_before's order), or the end: rank = t and
// the done flag when the score is at most thr (= tol kk), not positive or not finite.
// den2[0] = dc[p] + nugget and den2[1] = u[p], read here because zd_finish_kernel overwrites both
// while other workgroups still need them.  One workgroup of 256 threads.
__global__ __launch_bounds__(256) void zd_pick_kernel(PivcholState *st, double *den2,
                                                      const double *__restrict__ candv,
                                                      const int *__restrict__ candi, int nblk,
                                                      int t_step, double thr, double nugget,
                                                      const double *__restrict__ dc,
                                                      const double *__restrict__ u,
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
            den2[0] = dc[si[0]] + nugget, den2[1] = u[si[0]];
            piv[t_step] = si[0], gain[t_step] = g;
        } else {
            st->done = 1, st->rank = t_step;
        }
    }
}

// Step t's c with the new dc and u, and step t + 1's scores; grid ceil(Ap / 256).  Real rows (W:
// the workspace, ld; xc: the candidates' points): the nsl slices of the product in order, k(xc_a,
// xc_p) with gram_cross_kernel's arithmetic (g: the fit's parameters, its s^2 not used), the
// division by den = sqrt(dc[p] + nugget); c into column `col` of W; dc = fma(-c, c, dc) and
// u = fma(-c, u_p / den, u).  nugget = 0: c[p] = den with dc[p] and u[p] an exact 0, and a row taken
// earlier stores an exact 0 and keeps both.  Padding rows store 0 and are no candidates.
template <int D>
__global__ __launch_bounds__(256) void zd_finish_kernel(
    double *__restrict__ W, long ld, int col, int A, int Ap, const double *__restrict__ part,
    int nsl, const double *__restrict__ xc, GaussParams g, double nugget, const PivcholState *st,
    const double *__restrict__ den2, double *__restrict__ dc, double *__restrict__ u,
    int *__restrict__ taken, double *__restrict__ candv, int *__restrict__ candi)
{
    __shared__ double sv[256];
    __shared__ int si[256];
    if (st->done)
        return;
    const int t = threadIdx.x, p = st->p;
    const double den = sqrt(den2[0]), coef = den2[1] / den;
    const long i = (long)blockIdx.x * 256 + t;
    double v = -INFINITY;
    int idx = INT_MAX;
    if (i < Ap) {
        double cv = 0.0;
        if (i < A) {
            double s = 0.0;
            for (int y = 0; y < nsl; ++y)
                s += part[(long)y * ld + i];
            const double kv = g.c * exp_gauss(gauss_q<D>(xc + i * D, xc + (long)p * D, g));
            double di = dc[i], ui = u[i];
            int tk = taken[i];
            if (nugget == 0.0 && i == p) {
                cv = den, di = 0.0, ui = 0.0;
                taken[i] = tk = 1;
            } else if (nugget == 0.0 && tk) {
                di = 0.0;
            } else {
                cv = (kv - s) / den;
                di = __builtin_fma(-cv, cv, di);
                ui = __builtin_fma(-cv, coef, ui);
            }
            dc[i] = di, u[i] = ui;
            double sc;
            if (zd_score(ui, di, nugget, tk, &sc))
                v = sc, idx = (int)i;
        }
        W[i + (long)col * ld] = cv;
    }
    pivchol_wg_first(v, idx, sv, si);
    if (t == 0)
        candv[blockIdx.x] = sv[0], candi[blockIdx.x] = si[0];
}
