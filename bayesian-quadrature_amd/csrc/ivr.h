// ivr.h -- greedy designs that minimise the integrated posterior variance of a resident fit
// (fit.hip, bq_gp_ivr; include/bqhip.h has the contract).
// Part of the libbqhip.so kernel set; compiled into k_reduce.hip (host.h lists the units).
//
// R reference points with weights rho describe the measure, A candidates may be observed.  With
// T = Sigma(xc, xr) (Ap x Rp, ld Ap: a candidate's entries are a row, a load of T[:, j] is
// coalesced), dc = diag Sigma(xc, xc), dr = diag Sigma(xr, xr), step t is
//     score[a] = (sum_j rho_j T[a, j]^2) / (dc[a] + nugget)      the drop of sum_j rho_j dr[j]
//     p        = the first largest score
//     c        = (K(xc, xc_p) - W_c[:, :npad + t] W_c[p, :npad + t]^T) / sqrt(dc[p] + nugget)
//     u        = T[p, :] / sqrt(dc[p] + nugget)
//     T -= c u^T,  dc -= c o c,  dr -= u o u.
// W_c = [V_c | C_c] are the candidate rows of the prediction's workspace with the earlier c behind
// V, as in pivchol.h, whose pivchol_col_kernel forms the product.  Five launches a step, none of
// which waits for the host: the pivot, its score and the done flag live in a PivcholState on the
// device, dc[p] + nugget in a double beside it.
//   ivr_deflate_score_kernel  one pass over T, cut along j into slices of JS columns: step t - 1's
//                             rank-one update applied and stored, step t's numerators summed on
//                             the way: part[slice][a].  Step 0 neither updates nor stores.
//   ivr_score_kernel          the slices summed in order, the division, the eligibility rule, each
//                             workgroup's first candidate
//   ivr_pick_kernel           one workgroup: the argmax, the stop rule, piv[t], gain[t], the flag
//   pivchol_col_kernel        (pivchol.h) the row-gathered product over the candidate rows of W
//   ivr_column_kernel         c into column npad + t of W and its own buffer, dc, the taken rows;
//                             u gathered out of row p of T before T is touched again, dr
// After the last step T is not touched.  After the done flag every kernel returns at once.
//
// Determinism: JS comes from (Ap, Rp) alone (k_reduce.hip, ivr_plan), a slice's sum is
// BQ_PIVCHOL_U accumulators that take their j in ascending order and are folded in a fixed tree,
// the slices are added in ascending order, and the product over W is pivchol's: a step's bits
// depend on the shapes and on t, never on q.  No floating-point atomics.
#pragma once
#include "pivchol.h"

constexpr int BQ_IVR_JS_MAX = 512; // columns of T per slice at most: the pieces of u and rho in LDS

// dc = var on the A candidates, dr = var on the R reference points (0 on the padding of either);
// no row taken; workgroup 0: piv = -1, gain = 0, the state with rank = q.  dr == dc (the
// candidates are the reference points): one vector.  grid ceil(max(Ap, Rp) / 256).
__global__ __launch_bounds__(256) void ivr_init_kernel(const double *__restrict__ varc,
                                                       const double *__restrict__ varr, int A,
                                                       int Ap, int R, int Rp, int q,
                                                       PivcholState *st, double *den2,
                                                       long long *__restrict__ piv,
                                                       double *__restrict__ gain, double *dc,
                                                       double *dr, int *__restrict__ taken)
{
    const int t = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + t;
    if (i < Ap) {
        dc[i] = i < A ? varc[i] : 0.0;
        taken[i] = 0;
    }
    if (dr != dc && i < Rp)
        dr[i] = i < R ? varr[i] : 0.0;
    if (blockIdx.x == 0) {
        for (int k = t; k < q; k += 256)
            piv[k] = -1, gain[k] = 0.0;
        if (t == 0)
            st->done = 0, st->rank = q, st->p = 0, st->pad = 0, st->gain = 0.0, *den2 = 1.0;
    }
}

// *out = sum_j rho_j dr[j] over the Rp reference rows: thread t takes j = t, t + 256, .. in
// ascending order, then a fixed tree.  One workgroup of 256 threads.
__global__ __launch_bounds__(256) void ivr_ivar_kernel(const double *__restrict__ rho,
                                                       const double *__restrict__ dr, int Rp,
                                                       double *__restrict__ out)
{
    __shared__ double sv[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int j = t; j < Rp; j += 256)
        s = __builtin_fma(rho[j], dr[j], s);
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

// The pass over T (Ap x Rp, ld): part[slice y][a] = sum over j in the slice of rho_j T[a, j]^2,
// with UPD after T[a, j] <- fma(-c[a], u[j], T[a, j]) has been stored -- every entry of T is read
// once and written once a step.  grid (Ap / RB, Rp / JS), RB threads, one candidate each.  The
// slice's u and rho sit in LDS (every lane reads one address: a broadcast); BQ_PIVCHOL_U loads
// leave before the first use.  Rp and JS are multiples of 64, so a slice has whole groups of U.
template <int RB, bool UPD>
__global__ __launch_bounds__(RB) void ivr_deflate_score_kernel(
    double *__restrict__ T, long ld, int Rp, int JS, const PivcholState *st,
    const double *__restrict__ c, const double *__restrict__ u, const double *__restrict__ rho,
    double *__restrict__ part)
{
    constexpr int U = BQ_PIVCHOL_U;
    __shared__ double su[UPD ? BQ_IVR_JS_MAX : 1];
    __shared__ double sr[BQ_IVR_JS_MAX];
    if (st->done)
        return;
    const int t = threadIdx.x;
    const long a = (long)blockIdx.x * RB + t;
    const int j0 = (int)blockIdx.y * JS, len = min(JS, Rp - j0);
    for (int k = t; k < len; k += RB) {
        sr[k] = rho[j0 + k];
        if (UPD)
            su[k] = u[j0 + k];
    }
    __syncthreads();
    const double ca = UPD ? -c[a] : 0.0;
    double *w = T + a + (long)j0 * ld;
    double acc[U];
#pragma unroll
    for (int i = 0; i < U; ++i)
        acc[i] = 0.0;
    for (int k = 0; k + U <= len; k += U) {
        double v[U];
#pragma unroll
        for (int i = 0; i < U; ++i)
            v[i] = w[(long)(k + i) * ld];
        if (UPD) {
#pragma unroll
            for (int i = 0; i < U; ++i) {
                v[i] = __builtin_fma(ca, su[k + i], v[i]);
                w[(long)(k + i) * ld] = v[i];
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i)
            acc[i] = __builtin_fma(sr[k + i], v[i] * v[i], acc[i]);
    }
#pragma unroll
    for (int h = U / 2; h >= 1; h >>= 1)
#pragma unroll
        for (int i = 0; i < h; ++i)
            acc[i] += acc[i + h];
    part[(long)blockIdx.y * ld + a] = acc[0];
}

// Step t's scores and each workgroup's first candidate; grid ceil(Ap / 256).  A candidate is
// eligible iff dc + nugget > 0 and, with nugget = 0, it has not been taken; the others and the
// padding are no candidates.  score0 (step 0 alone, else NULL): the scores, 0 where ineligible.
__global__ __launch_bounds__(256) void ivr_score_kernel(
    const double *__restrict__ part, long ld, int nsl, int A, const double *__restrict__ dc,
    const int *__restrict__ taken, double nugget, const PivcholState *st,
    double *__restrict__ score0, double *__restrict__ candv, int *__restrict__ candi)
{
    __shared__ double sv[256];
    __shared__ int si[256];
    if (st->done)
        return;
    const int t = threadIdx.x;
    const long a = (long)blockIdx.x * 256 + t;
    double v = -INFINITY;
    int idx = INT_MAX;
    if (a < A) {
        double s = 0.0;
        for (int y = 0; y < nsl; ++y)
            s += part[(long)y * ld + a];
        const double den2 = dc[a] + nugget;
        const bool ok = den2 > 0.0 && !(nugget == 0.0 && taken[a]);
        const double sc = ok ? s / den2 : 0.0;
        if (score0)
            score0[a] = sc;
        if (ok)
            v = sc, idx = (int)a;
    }
    pivchol_wg_first(v, idx, sv, si);
    if (t == 0)
        candv[blockIdx.x] = sv[0], candi[blockIdx.x] = si[0];
}

// Step t's pivot out of the nblk candidates (pivchol_before's order), or the end: rank = t and
// the done flag when the score is at most thr (= tol k0 sum rho), not positive or not finite.
// *den2 = dc[p] + nugget, read here because ivr_column_kernel overwrites dc[p] while other
// workgroups still need it.  One workgroup of 256 threads.
__global__ __launch_bounds__(256) void ivr_pick_kernel(PivcholState *st, double *den2,
                                                       const double *__restrict__ candv,
                                                       const int *__restrict__ candi, int nblk,
                                                       int t_step, double thr, double nugget,
                                                       const double *__restrict__ dc,
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
            *den2 = dc[si[0]] + nugget;
            piv[t_step] = si[0], gain[t_step] = g;
        } else {
            st->done = 1, st->rank = t_step;
        }
    }
}

// Step t's c and u.  grid ceil(Ap / 256) + ceil(Rp / 256): the first nbc workgroups take the
// candidates, the others the reference points.
// Candidates (W: their rows of the workspace, ld; xc: their points): the nsl slices of the
// product in order, k(xc_a, xc_p) with gram_cross_kernel's arithmetic (g: the fit's parameters,
// its s^2 not used), the division by den = sqrt(dc[p] + nugget); c into column `col` of W and
// into cb; dc.  nugget = 0: c[p] = den and dc[p] an exact 0, and a row taken earlier stores an
// exact 0 and keeps dc = 0.  Padding rows store 0.
// Reference points: u[j] = T[p, j] / den into ub, dr[j] = fma(-u, u, dr[j]) (dr == NULL: the
// candidates are the reference points, dc is their variance).
template <int D>
__global__ __launch_bounds__(256) void ivr_column_kernel(
    double *__restrict__ W, long ld, int col, int A, int Ap, int nbc,
    const double *__restrict__ part, int nsl, const double *__restrict__ xc, GaussParams g,
    double nugget, const PivcholState *st, const double *__restrict__ den2,
    double *__restrict__ dc, int *__restrict__ taken, double *__restrict__ cb,
    const double *__restrict__ T, int Rp, double *__restrict__ ub, double *__restrict__ dr)
{
    if (st->done)
        return;
    const int t = threadIdx.x, p = st->p;
    const double den = sqrt(*den2);
    if ((int)blockIdx.x >= nbc) {
        const long j = (long)(blockIdx.x - nbc) * 256 + t;
        if (j < Rp) {
            const double uj = T[p + j * (long)Ap] / den;
            ub[j] = uj;
            if (dr)
                dr[j] = __builtin_fma(-uj, uj, dr[j]);
        }
        return;
    }
    const long i = (long)blockIdx.x * 256 + t;
    if (i >= Ap)
        return;
    double cv = 0.0;
    if (i < A) {
        double s = 0.0;
        for (int y = 0; y < nsl; ++y)
            s += part[(long)y * ld + i];
        const double kv = g.c * exp_gauss(gauss_q<D>(xc + i * D, xc + (long)p * D, g));
        double di = dc[i];
        if (nugget == 0.0 && i == p) {
            cv = den, di = 0.0;
            taken[i] = 1;
        } else if (nugget == 0.0 && taken[i]) {
            di = 0.0;
        } else {
            cv = (kv - s) / den;
            di = __builtin_fma(-cv, cv, di);
        }
        dc[i] = di;
    }
    W[i + (long)col * ld] = cv;
    cb[i] = cv;
}
