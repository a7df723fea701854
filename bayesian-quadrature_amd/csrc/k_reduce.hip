// k_reduce.hip -- read-outs, single-vector sweeps and small utilities (reduce.h, trsv.h), the
// posterior's gradients at the query points (pgrad.h), the kernels that grow and shrink a
// resident fit (append.h, remove.h), the posterior samples' normals and triangular product
// (sample.h), the pivoted partial Cholesky of a posterior (pivchol.h), the designs that minimise
// the integrated variance (ivr.h), the integral of a fit and the designs that lower its variance
// (zdesign.h), the pair sums of square-root-warped quadrature (sqwarp.h), the polynomial trend of a
// fit (trend.h) and their launchers.
#include "host.h"
#include "reduce.h"
#include "pgrad.h"
#include "sample.h"
#include "pivchol.h"
#include "ivr.h"
#include "zdesign.h"
#include "sqwarp.h"
#include "trend.h"
#include "trsv.h"
#include "trsvflow.h"
#include "append.h"
#include "remove.h"

namespace bqh {

int launch_finalize(bq_ctx *c, const double *A, long lda, long astride, Layout L, double *scal,
                    double *mean, double *var, long mstride, int batch, double work)
{
    Bracket br(c, BQ_K_REDUCE, work);
    hipLaunchKernelGGL(finalize_kernel, dim3(1, 1, batch), dim3(256), 0, c->stream, A, lda, astride,
                       L, scal, mean, var, mstride);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_plan_readout(bq_ctx *c, const double *A, long lda, long astride, Layout L,
                        const GaussParams *gp, double *scal, double *mean, double *var,
                        long mstride, int batch)
{
    Bracket br(c, BQ_K_REDUCE, 8.0 * (L.M + 1.0) * L.npad * batch);
    hipLaunchKernelGGL(plan_readout_kernel, dim3((L.M + 16) / 16, 1, batch), dim3(1024), 0,
                       c->stream, A, lda, astride, L, gp, scal, mean, var, mstride);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// mean_i = v_i . z, var_i = k0 - |v_i|^2 over the Mp (multiple of 16) rows of V
int launch_rowdot(bq_ctx *c, const double *V, long ldv, int M, int Mp, int npad, const double *z,
                  double k0, double *mean, double *var, long zstride)
{
    Bracket br(c, BQ_K_REDUCE);
    hipLaunchKernelGGL(rowdot_kernel, dim3(Mp / 16), dim3(1024), 0, c->stream, V, ldv, M, npad, z,
                       zstride, k0, mean, var);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_predict_mean(bq_ctx *c, int d, const double *xo, int M, const double *pts, int n,
                        const double *alpha, const GaussParams &g, double *mean)
{
    Bracket br(c, BQ_K_REDUCE);
    dim3 grid((unsigned)((M + 3) / 4));
    BQ_DISPATCH_D(d, hipLaunchKernelGGL(predict_mean_kernel<D>, grid, dim3(256), 0, c->stream, xo, M,
                                        pts, n, alpha, g, mean));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// dmean, dvar (d x M each, entry [k + j d]) from beta (Mp x npad, ld ldb; nullptr: no dvar) and
// alpha (nullptr: no dmean) over the Mp (multiple of 16) rows of beta
int launch_predict_grad(bq_ctx *c, int d, const double *beta, long ldb, int M, int Mp,
                        const double *xo, const double *pts, int n, const double *alpha,
                        const GaussParams &g, double *dmean, double *dvar)
{
    Bracket br(c, BQ_K_REDUCE);
    dim3 grid((unsigned)(Mp / 16));
    BQ_DISPATCH_D(d, hipLaunchKernelGGL(predict_grad_kernel<D>, grid, dim3(1024), 0, c->stream, beta,
                                        ldb, M, xo, pts, n, alpha, g, dmean, dvar));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// the fused mean route: mean (M; may be nullptr) and dmean (d x M) in one launch
int launch_predict_mean_grad(bq_ctx *c, int d, const double *xo, int M, const double *pts, int n,
                             const double *alpha, const GaussParams &g, double *mean,
                             double *dmean)
{
    Bracket br(c, BQ_K_REDUCE);
    dim3 grid((unsigned)((M + 3) / 4));
    BQ_DISPATCH_D(d, hipLaunchKernelGGL(predict_mean_grad_kernel<D>, grid, dim3(256), 0, c->stream, xo,
                                        M, pts, n, alpha, g, mean, dmean));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// ---- posterior samples (sample.h; fit.hip, bq_gp_sample) ----
// Z (Mp x S, ld ldz): standard normals keyed by (seed, j + M s) in rows < M, zeros below
int launch_normal_fill(bq_ctx *c, double *Z, long ldz, int M, int Mp, int S, uint64_t seed)
{
    Bracket br(c, BQ_K_REDUCE);
    const long total = (long)Mp * S;
    hipLaunchKernelGGL(normal_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       c->stream, Z, ldz, M, Mp, S, seed);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// A[i, i] += add for i < M, = 1 for M <= i < Mp
int launch_sample_diag(bq_ctx *c, double *A, long lda, int M, int Mp, double add)
{
    hipLaunchKernelGGL(sample_diag_kernel, dim3((Mp + 255) / 256), dim3(256), 0, c->stream, A, lda,
                       M, Mp, add);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// out (M x S, ld ldo) = mean 1^T + tril(L) Z; L: Mp x Mp, Z: Mp x S with zero rows M .. Mp
int launch_tri_sample(bq_ctx *c, const double *L, long ldl, const double *Z, long ldz,
                      const double *mean, double *out, long ldo, int M, int Mp, int S)
{
    if (M < 1 || S < 1 || Mp < M || (Mp & 63))
        return fail(c, BQ_ERR_BAD_ARG, "tri_sample: M, S >= 1 over whole 64-row blocks");
    Bracket br(c, BQ_K_GEMM, (double)Mp * Mp * S);
    hipLaunchKernelGGL(tri_sample_kernel, dim3(Mp / 64, (S + 63) / 64), dim3(256), 0, c->stream, L,
                       ldl, Z, ldz, mean, out, ldo, M, S);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// ---- pivoted partial Cholesky of a posterior (pivchol.h; fit.hip, bq_gp_pivchol) ----
// The shape of q steps over Mp rows behind npad columns of V, from (Mp, npad) alone but for the
// sizes that q sets: rows per workgroup of the column kernel (64 below 16384 rows, so that small M
// still fills the chip by slices), columns per slice (about 1024 workgroups at step 0, whole
// 64-column blocks, 64 .. BQ_PIVCHOL_KS_MAX), and the places of the workspace's parts, in doubles.
PivcholPlan pivchol_plan(int Mp, int npad, int q)
{
    auto granule = [](size_t doubles) { return (doubles + 31) & ~(size_t)31; };
    PivcholPlan pl{};
    pl.rb = (Mp >= 16384 && (Mp % 256) == 0) ? 256 : 64;
    const long want = (1024 + Mp / pl.rb - 1) / (Mp / pl.rb);
    pl.ks = (int)std::min<long>(BQ_PIVCHOL_KS_MAX, std::max<long>(64, npad / want / 64 * 64));
    pl.nblk = (Mp + 255) / 256;
    pl.nsl = (npad + q - 1 + pl.ks - 1) / pl.ks; // slices of the last step's npad + q - 1 columns
    pl.o_gain = granule((sizeof(PivcholState) + 7) / 8);
    pl.o_piv = pl.o_gain + (size_t)q;
    pl.o_d = pl.o_piv + (size_t)q;
    pl.head = pl.o_d + (size_t)Mp;
    pl.o_taken = granule(pl.head);
    pl.o_candv = pl.o_taken + granule(((size_t)Mp + 1) / 2);
    pl.o_candi = pl.o_candv + granule((size_t)pl.nblk);
    pl.o_part = pl.o_candi + granule(((size_t)pl.nblk + 1) / 2);
    pl.total = pl.o_part + (size_t)pl.nsl * Mp;
    return pl;
}

// d = var, nothing taken, the state, piv = -1 and gain = 0, then step 0's pivot
int launch_pivchol_init(bq_ctx *c, const PivcholPlan &pl, double *ws, const double *var, int M,
                        int Mp, int q, double thr)
{
    PivcholState *st = reinterpret_cast<PivcholState *>(ws);
    long long *piv = reinterpret_cast<long long *>(ws + pl.o_piv);
    int *taken = reinterpret_cast<int *>(ws + pl.o_taken);
    int *candi = reinterpret_cast<int *>(ws + pl.o_candi);
    Bracket br(c, BQ_K_REDUCE, 16.0 * Mp);
    hipLaunchKernelGGL(pivchol_init_kernel, dim3(pl.nblk), dim3(256), 0, c->stream, var, M, Mp, q,
                       st, piv, ws + pl.o_gain, ws + pl.o_d, taken, ws + pl.o_candv, candi);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(pivchol_select_kernel, dim3(1), dim3(256), 0, c->stream, st,
                       ws + pl.o_candv, candi, pl.nblk, 0, thr, piv, ws + pl.o_gain);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// step j < q: column npad + j of W (Mp x (npad + q), ld Mp) and the new d; then, for j + 1 < q,
// step j + 1's pivot.  xq: the d x M points; g: the fit's kernel parameters
int launch_pivchol_step(bq_ctx *c, const PivcholPlan &pl, double *ws, double *W, int d,
                        const double *xq, const GaussParams &g, int M, int Mp, int npad, int q,
                        int j, double nugget, double thr)
{
    if (M < 1 || Mp < M || (Mp & 63) || j < 0 || j >= q || npad < 0)
        return fail(c, BQ_ERR_BAD_ARG, "pivchol: step %d of %d over %d rows", j, q, M);
    if (d < 1 || d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    PivcholState *st = reinterpret_cast<PivcholState *>(ws);
    long long *piv = reinterpret_cast<long long *>(ws + pl.o_piv);
    int *taken = reinterpret_cast<int *>(ws + pl.o_taken);
    int *candi = reinterpret_cast<int *>(ws + pl.o_candi);
    double *part = ws + pl.o_part;
    const int K = npad + j, nsl = (K + pl.ks - 1) / pl.ks;
    const long ld = Mp;
    if (nsl > 0) {
        Bracket br(c, BQ_K_REDUCE, 8.0 * Mp * K);
        const dim3 grid((unsigned)(Mp / pl.rb), (unsigned)nsl);
        if (pl.rb == 256)
            hipLaunchKernelGGL(pivchol_col_kernel<256>, grid, dim3(256), 0, c->stream, W, ld, K,
                               pl.ks, st, part);
        else
            hipLaunchKernelGGL(pivchol_col_kernel<64>, grid, dim3(64), 0, c->stream, W, ld, K, pl.ks,
                               st, part);
        HIPCHK(c, hipGetLastError());
    }
    {
        Bracket br(c, BQ_K_REDUCE, 8.0 * Mp * (nsl + 3.0));
        BQ_DISPATCH_D(d, hipLaunchKernelGGL(pivchol_finish_kernel<D>, dim3(pl.nblk), dim3(256), 0,
                                            c->stream, W, ld, K, M, Mp, part, nsl, xq, g, nugget, st,
                                            ws + pl.o_d, taken, ws + pl.o_candv, candi));
        HIPCHK(c, hipGetLastError());
    }
    if (j + 1 < q) {
        hipLaunchKernelGGL(pivchol_select_kernel, dim3(1), dim3(256), 0, c->stream, st,
                           ws + pl.o_candv, candi, pl.nblk, j + 1, thr, piv, ws + pl.o_gain);
        HIPCHK(c, hipGetLastError());
    }
    return BQ_OK;
}

// ---- designs that minimise the integrated posterior variance (ivr.h; fit.hip, bq_gp_ivr) ----
// The shape of q steps.  The joint point set is [reference points, padded to Rp | candidates], so
// that the candidate rows of W start on a 64-row boundary; self: the candidates alone.  The pass
// over T is shaped like pivchol's product, from (Ap, Rp) alone: 256 candidates per workgroup from
// 16384 on, 64 below so that few candidates still fill the chip by slices; about 1024 workgroups,
// whole 64-column blocks, 64 .. BQ_IVR_JS_MAX columns per slice.  The product over the candidate
// rows of W is pivchol_plan's for Ap rows.
IvrPlan ivr_plan(int A, int R, bool self, int npad, int q)
{
    auto granule = [](size_t doubles) { return (doubles + 31) & ~(size_t)31; };
    IvrPlan pl{};
    pl.A = A, pl.R = self ? A : R, pl.self = self, pl.npad = npad, pl.q = q;
    pl.Ap = (A + 63) / 64 * 64;
    pl.Rp = self ? pl.Ap : (R + 63) / 64 * 64;
    pl.cand0 = self ? 0 : pl.Rp;
    pl.Mp = pl.cand0 + pl.Ap;
    pl.rb = (pl.Ap >= 16384 && (pl.Ap % 256) == 0) ? 256 : 64;
    const long want = (1024 + pl.Ap / pl.rb - 1) / (pl.Ap / pl.rb);
    pl.js = (int)std::min<long>(BQ_IVR_JS_MAX, std::max<long>(64, pl.Rp / want / 64 * 64));
    pl.nsl = (pl.Rp + pl.js - 1) / pl.js;
    pl.nblk = (pl.Ap + 255) / 256;
    const PivcholPlan pw = pivchol_plan(pl.Ap, npad, q);
    pl.wrb = pw.rb, pl.wks = pw.ks, pl.wnsl = pw.nsl;
    pl.o_den = granule((sizeof(PivcholState) + 7) / 8);
    pl.o_ivar = pl.o_den + 1;
    pl.o_gain = pl.o_ivar + 1;
    pl.o_piv = pl.o_gain + (size_t)q;
    pl.o_dc = pl.o_piv + (size_t)q;
    pl.o_dr = self ? pl.o_dc : pl.o_dc + (size_t)pl.Ap;
    pl.o_score0 = pl.o_dr + (size_t)pl.Rp;
    pl.head = pl.o_score0 + (size_t)pl.Ap;
    pl.o_taken = granule(pl.head);
    pl.o_candv = pl.o_taken + granule(((size_t)pl.Ap + 1) / 2);
    pl.o_candi = pl.o_candv + granule((size_t)pl.nblk);
    pl.o_c = pl.o_candi + granule(((size_t)pl.nblk + 1) / 2);
    pl.o_u = pl.o_c + (size_t)pl.Ap;
    pl.o_rho = pl.o_u + (size_t)pl.Rp;
    pl.o_part = pl.o_rho + (size_t)pl.Rp;
    pl.o_wpart = pl.o_part + (size_t)pl.nsl * pl.Ap;
    pl.total = pl.o_wpart + (size_t)pl.wnsl * pl.Mp;
    return pl;
}

// dc, dr = the sweep's variances (var: Mp of them, the joint set's), nothing taken, the state,
// piv = -1 and gain = 0; then sum rho dr.  rho is in the workspace already.
int launch_ivr_init(bq_ctx *c, const IvrPlan &pl, double *ws, const double *var)
{
    PivcholState *st = reinterpret_cast<PivcholState *>(ws);
    long long *piv = reinterpret_cast<long long *>(ws + pl.o_piv);
    int *taken = reinterpret_cast<int *>(ws + pl.o_taken);
    Bracket br(c, BQ_K_REDUCE, 16.0 * pl.Mp);
    hipLaunchKernelGGL(ivr_init_kernel, dim3((std::max(pl.Ap, pl.Rp) + 255) / 256), dim3(256), 0,
                       c->stream, var + pl.cand0, var, pl.A, pl.Ap, pl.R, pl.Rp, pl.q, st,
                       ws + pl.o_den, piv, ws + pl.o_gain, ws + pl.o_dc, ws + pl.o_dr, taken);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(ivr_ivar_kernel, dim3(1), dim3(256), 0, c->stream, ws + pl.o_rho,
                       ws + pl.o_dr, pl.Rp, ws + pl.o_ivar);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// step t < q: the pass over T (Ap x Rp, ld Ap) that applies step t - 1's update and sums step t's
// numerators, the scores and the pivot, then c (column npad + t of the candidate rows of W, Mp x
// (npad + q), ld Mp) and u with the new dc and dr.  xc: the candidates' points; g: the fit's
// kernel parameters
int launch_ivr_step(bq_ctx *c, const IvrPlan &pl, double *ws, double *T, double *W, int d,
                    const double *xc, const GaussParams &g, int t, double nugget, double thr)
{
    if (pl.A < 1 || pl.R < 1 || t < 0 || t >= pl.q || (pl.Rp & 63) || (pl.js & 63) ||
        pl.js > BQ_IVR_JS_MAX || (pl.Ap % pl.rb))
        return fail(c, BQ_ERR_BAD_ARG, "ivr: step %d of %d over %d candidates", t, pl.q, pl.A);
    if (d < 1 || d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    PivcholState *st = reinterpret_cast<PivcholState *>(ws);
    long long *piv = reinterpret_cast<long long *>(ws + pl.o_piv);
    int *taken = reinterpret_cast<int *>(ws + pl.o_taken);
    int *candi = reinterpret_cast<int *>(ws + pl.o_candi);
    double *part = ws + pl.o_part, *wpart = ws + pl.o_wpart, *cb = ws + pl.o_c, *ub = ws + pl.o_u;
    double *Wc = W + pl.cand0;
    const long ldt = pl.Ap, ldw = pl.Mp;
    {
        Bracket br(c, BQ_K_REDUCE, (t ? 16.0 : 8.0) * pl.Ap * pl.Rp);
        const dim3 grid((unsigned)(pl.Ap / pl.rb), (unsigned)pl.nsl);
#define BQ_IVR_PASS(RB, UPD)                                                                      \
    hipLaunchKernelGGL((ivr_deflate_score_kernel<RB, UPD>), grid, dim3(RB), 0, c->stream, T, ldt,   \
                       pl.Rp, pl.js, st, cb, ub, ws + pl.o_rho, part)
        if (pl.rb == 256 && t)
            BQ_IVR_PASS(256, true);
        else if (pl.rb == 256)
            BQ_IVR_PASS(256, false);
        else if (t)
            BQ_IVR_PASS(64, true);
        else
            BQ_IVR_PASS(64, false);
#undef BQ_IVR_PASS
        HIPCHK(c, hipGetLastError());
    }
    {
        Bracket br(c, BQ_K_REDUCE, 8.0 * pl.Ap * (pl.nsl + 2.0));
        hipLaunchKernelGGL(ivr_score_kernel, dim3(pl.nblk), dim3(256), 0, c->stream, part, ldt,
                           pl.nsl, pl.A, ws + pl.o_dc, taken, nugget, st,
                           t == 0 ? ws + pl.o_score0 : nullptr, ws + pl.o_candv, candi);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(ivr_pick_kernel, dim3(1), dim3(256), 0, c->stream, st, ws + pl.o_den,
                           ws + pl.o_candv, candi, pl.nblk, t, thr, nugget, ws + pl.o_dc, piv,
                           ws + pl.o_gain);
        HIPCHK(c, hipGetLastError());
    }
    const int K = pl.npad + t, wnsl = (K + pl.wks - 1) / pl.wks;
    if (wnsl > 0) {
        Bracket br(c, BQ_K_REDUCE, 8.0 * pl.Ap * K);
        const dim3 grid((unsigned)(pl.Ap / pl.wrb), (unsigned)wnsl);
        if (pl.wrb == 256)
            hipLaunchKernelGGL(pivchol_col_kernel<256>, grid, dim3(256), 0, c->stream, Wc, ldw, K,
                               pl.wks, st, wpart);
        else
            hipLaunchKernelGGL(pivchol_col_kernel<64>, grid, dim3(64), 0, c->stream, Wc, ldw, K,
                               pl.wks, st, wpart);
        HIPCHK(c, hipGetLastError());
    }
    {
        Bracket br(c, BQ_K_REDUCE, 8.0 * (pl.Ap * (wnsl + 4.0) + 3.0 * pl.Rp));
        const int nbr = (pl.Rp + 255) / 256;
        BQ_DISPATCH_D(d, hipLaunchKernelGGL(ivr_column_kernel<D>, dim3(pl.nblk + nbr), dim3(256), 0,
                                            c->stream, Wc, ldw, K, pl.A, pl.Ap, pl.nblk, wpart, wnsl,
                                            xc, g, nugget, st, ws + pl.o_den, ws + pl.o_dc, taken, cb,
                                            T, pl.Rp, ub, pl.self ? nullptr : ws + pl.o_dr));
        HIPCHK(c, hipGetLastError());
    }
    return BQ_OK;
}

// ---- the integral of a fit and the designs that lower its variance (zdesign.h; fit.hip,
// bq_gp_integral, bq_gp_zdesign) ----
// The shape of q steps over A candidates: the product over the Ap rows of W is pivchol_plan's, and
// so are the workgroups of the vector kernels.
ZdPlan zd_plan(int A, int npad, int q)
{
    auto granule = [](size_t doubles) { return (doubles + 31) & ~(size_t)31; };
    ZdPlan pl{};
    pl.A = A, pl.npad = npad, pl.q = q;
    pl.Ap = (A + 63) / 64 * 64;
    const PivcholPlan pw = pivchol_plan(pl.Ap, npad, q);
    pl.rb = pw.rb, pl.ks = pw.ks, pl.nsl = pw.nsl, pl.nblk = pw.nblk;
    pl.o_den = granule((sizeof(PivcholState) + 7) / 8);
    pl.o_gain = pl.o_den + 2;
    pl.o_piv = pl.o_gain + (size_t)q;
    pl.o_dc = pl.o_piv + (size_t)q;
    pl.o_u = pl.o_dc + (size_t)pl.Ap;
    pl.o_score0 = pl.o_u + (size_t)pl.Ap;
    pl.head = pl.o_score0 + (size_t)pl.Ap;
    pl.o_taken = granule(pl.head);
    pl.o_candv = pl.o_taken + granule(((size_t)pl.Ap + 1) / 2);
    pl.o_candi = pl.o_candv + granule((size_t)pl.nblk);
    pl.o_kap = pl.o_candi + granule(((size_t)pl.nblk + 1) / 2);
    pl.o_part = pl.o_kap + (size_t)pl.Ap;
    pl.total = pl.o_part + (size_t)pl.nsl * pl.Ap;
    return pl;
}

int launch_zd_dot(bq_ctx *c, const double *a, const double *b, int n, double *out)
{
    hipLaunchKernelGGL(zd_dot_kernel, dim3(1), dim3(256), 0, c->stream, a, b, n, out);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// V b over the npad columns of V = W (Ap x npad, ld Ap) in the product's slices; dc = var (Ap of
// them, the sweep's) and u = kappa(xc) - V b (kappa in the workspace already), nothing taken, the
// state, piv = -1 and gain = 0, step 0's scores; then step 0's pivot
int launch_zd_start(bq_ctx *c, const ZdPlan &pl, double *ws, const double *W, const double *b,
                    const double *var, double nugget, double thr)
{
    if (pl.A < 1 || pl.q < 1 || pl.npad < 1 || (pl.Ap & 63) || (pl.Ap % pl.rb) ||
        pl.ks > BQ_PIVCHOL_KS_MAX)
        return fail(c, BQ_ERR_BAD_ARG, "zdesign: %d steps over %d candidates", pl.q, pl.A);
    const long ld = pl.Ap;
    const int nsl0 = (pl.npad + pl.ks - 1) / pl.ks; // <= pl.nsl, the slices of npad + q - 1 columns
    {
        Bracket br(c, BQ_K_REDUCE, 8.0 * pl.Ap * pl.npad);
        const dim3 grid((unsigned)(pl.Ap / pl.rb), (unsigned)nsl0);
        if (pl.rb == 256)
            hipLaunchKernelGGL(zd_vb_kernel<256>, grid, dim3(256), 0, c->stream, W, ld, pl.npad,
                               pl.ks, b, ws + pl.o_part);
        else
            hipLaunchKernelGGL(zd_vb_kernel<64>, grid, dim3(64), 0, c->stream, W, ld, pl.npad, pl.ks,
                               b, ws + pl.o_part);
        HIPCHK(c, hipGetLastError());
    }
    PivcholState *st = reinterpret_cast<PivcholState *>(ws);
    long long *piv = reinterpret_cast<long long *>(ws + pl.o_piv);
    int *taken = reinterpret_cast<int *>(ws + pl.o_taken);
    int *candi = reinterpret_cast<int *>(ws + pl.o_candi);
    Bracket br(c, BQ_K_REDUCE, 48.0 * pl.Ap);
    hipLaunchKernelGGL(zd_start_kernel, dim3(pl.nblk), dim3(256), 0, c->stream, var, ws + pl.o_kap,
                       ws + pl.o_part, ld, nsl0, pl.A, pl.Ap, pl.q, nugget, st, ws + pl.o_den, piv,
                       ws + pl.o_gain, ws + pl.o_dc, ws + pl.o_u, taken, ws + pl.o_score0,
                       ws + pl.o_candv, candi);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(zd_pick_kernel, dim3(1), dim3(256), 0, c->stream, st, ws + pl.o_den,
                       ws + pl.o_candv, candi, pl.nblk, 0, thr, nugget, ws + pl.o_dc, ws + pl.o_u,
                       piv, ws + pl.o_gain);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// step t < q: c (column npad + t of W, Ap x (npad + q), ld Ap) with the new dc and u; then, for
// t + 1 < q, step t + 1's pivot.  xc: the candidates' points; g: the fit's kernel parameters
int launch_zd_step(bq_ctx *c, const ZdPlan &pl, double *ws, double *W, int d, const double *xc,
                   const GaussParams &g, int t, double nugget, double thr)
{
    if (pl.A < 1 || t < 0 || t >= pl.q || pl.npad < 0 || (pl.Ap & 63) || (pl.Ap % pl.rb) ||
        pl.ks > BQ_PIVCHOL_KS_MAX)
        return fail(c, BQ_ERR_BAD_ARG, "zdesign: step %d of %d over %d candidates", t, pl.q, pl.A);
    if (d < 1 || d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    PivcholState *st = reinterpret_cast<PivcholState *>(ws);
    long long *piv = reinterpret_cast<long long *>(ws + pl.o_piv);
    int *taken = reinterpret_cast<int *>(ws + pl.o_taken);
    int *candi = reinterpret_cast<int *>(ws + pl.o_candi);
    double *part = ws + pl.o_part;
    const int K = pl.npad + t, nsl = (K + pl.ks - 1) / pl.ks;
    const long ld = pl.Ap;
    if (nsl > 0) {
        Bracket br(c, BQ_K_REDUCE, 8.0 * pl.Ap * K);
        const dim3 grid((unsigned)(pl.Ap / pl.rb), (unsigned)nsl);
        if (pl.rb == 256)
            hipLaunchKernelGGL(pivchol_col_kernel<256>, grid, dim3(256), 0, c->stream, W, ld, K,
                               pl.ks, st, part);
        else
            hipLaunchKernelGGL(pivchol_col_kernel<64>, grid, dim3(64), 0, c->stream, W, ld, K, pl.ks,
                               st, part);
        HIPCHK(c, hipGetLastError());
    }
    {
        Bracket br(c, BQ_K_REDUCE, 8.0 * pl.Ap * (nsl + 5.0));
        BQ_DISPATCH_D(d, hipLaunchKernelGGL(zd_finish_kernel<D>, dim3(pl.nblk), dim3(256), 0,
                                            c->stream, W, ld, K, pl.A, pl.Ap, part, nsl, xc, g, nugget,
                                            st, ws + pl.o_den, ws + pl.o_dc, ws + pl.o_u, taken,
                                            ws + pl.o_candv, candi));
        HIPCHK(c, hipGetLastError());
    }
    if (t + 1 < pl.q) {
        hipLaunchKernelGGL(zd_pick_kernel, dim3(1), dim3(256), 0, c->stream, st, ws + pl.o_den,
                           ws + pl.o_candv, candi, pl.nblk, t + 1, thr, nugget, ws + pl.o_dc,
                           ws + pl.o_u, piv, ws + pl.o_gain);
        HIPCHK(c, hipGetLastError());
    }
    return BQ_OK;
}

// ---- square-root-warped quadrature of a fit (sqwarp.h; fit.hip, bq_gp_sqintegral,
// bq_gp_sqdesign) ----
// The column slices of a pair sum of R rows (ldp of them stored) against n columns, from the shapes
// alone: the row blocks by themselves where they give every CU eight workgroups (2048 of them:
// the kernel is bound by its arithmetic, and with two workgroups per CU it ran at 0.50-0.64e12
// pairs a second, LABBOOK), else as many slices of whole tiles as reach that, at most
// BQ_SQ_MAX_SLICES.
SqPlan sq_pair_plan(long ldp, int n)
{
    SqPlan pl{};
    const long rblk = (ldp + BQ_SQ_RB - 1) / BQ_SQ_RB;
    const int tiles = std::max(1, (n + BQ_SQ_TJ - 1) / BQ_SQ_TJ);
    long want = rblk >= 2048 ? 1 : (2048 + rblk - 1) / std::max(1L, rblk);
    want = std::min<long>({want, (long)tiles, (long)BQ_SQ_MAX_SLICES});
    pl.js = (int)((tiles + want - 1) / want) * BQ_SQ_TJ;
    pl.nsl = std::max(1, (n + pl.js - 1) / pl.js);
    return pl;
}

// the coordinates of the n points x (d x n) into t (np x (d or 2 d)) and their weights into wt (np,
// or NULL): `sums` -- the 2 d coordinates of W with weight alpha; else the d difference
// coordinates of Q with weight alpha times the point's Gaussian factor.  alpha NULL: weight 1
int launch_sq_xform(bq_ctx *c, int d, bool sums, const double *x, int n, int np, const SqForms &f,
                    const double *alpha, double *t, double *wt)
{
    if (d < 1 || d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    if (n < 0 || np < n || np < 1)
        return fail(c, BQ_ERR_BAD_ARG, "sqwarp: %d points in %d places", n, np);
    const dim3 grid((unsigned)((np + 255) / 256));
    BQ_DISPATCH_D(d, {
        SqXform<D> g{};
        for (int k = 0; k < D * D; ++k) {
            g.a1[k] = sums ? f.a1w[k] : f.a1q[k];
            g.a2[k] = f.a2w[k];
            g.kl[k] = f.kl[k];
        }
        for (int k = 0; k < D; ++k)
            g.m2[k] = g.km[k] = f.mu[k];
        g.klogc = f.klogc;
        if (sums)
            hipLaunchKernelGGL((sq_xform_kernel<D, D>), grid, dim3(256), 0, c->stream, x, n, np, g,
                               alpha, t, wt);
        else
            hipLaunchKernelGGL((sq_xform_kernel<D, 0>), grid, dim3(256), 0, c->stream, x, n, np, g,
                               alpha, t, wt);
    });
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// out[a] = scale sum_j pair(tp_a, tx_j) wt_j for the R row points (Rp entries of out, zero from R
// on) against the n column points; part: sq_pair_plan(Rp, n).nsl x Rp doubles
int launch_sq_pair(bq_ctx *c, int d, bool sums, const double *tp, int R, int Rp, const double *tx,
                   const double *wt, int n, double scale, double *part, double *out)
{
    if (d < 1 || d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    if (R < 1 || Rp < R || n < 1)
        return fail(c, BQ_ERR_BAD_ARG, "sqwarp: %d of %d rows against %d columns", R, Rp, n);
    const SqPlan pl = sq_pair_plan(Rp, n);
    const long ldp = Rp;
    {
        Bracket br(c, BQ_K_REDUCE, (double)R * n);
        const dim3 grid((unsigned)((Rp + BQ_SQ_RB - 1) / BQ_SQ_RB), (unsigned)pl.nsl);
        BQ_DISPATCH_D(d, {
            if (sums)
                hipLaunchKernelGGL((sq_pair_kernel<D, D>), grid, dim3(BQ_SQ_RB), 0, c->stream, tp, R,
                                   ldp, tx, wt, n, pl.js, part);
            else
                hipLaunchKernelGGL((sq_pair_kernel<D, 0>), grid, dim3(BQ_SQ_RB), 0, c->stream, tp, R,
                                   ldp, tx, wt, n, pl.js, part);
        });
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(sq_fold_kernel, dim3((unsigned)((Rp + 255) / 256)), dim3(256), 0, c->stream,
                       part, ldp, pl.nsl, R, Rp, scale, out);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// ---- the polynomial trend of a fit (trend.h; fit.hip, bq_gp_trend, bq_gp_predict_trend) ----
// The places of the state's parts, from npad alone: the slices are the 64-column blocks of G, and
// the partial sums have room for the largest basis, so that a call with another key reuses them.
TrendPlan trend_plan(int npad)
{
    auto granule = [](size_t doubles) { return (doubles + 31) & ~(size_t)31; };
    constexpr size_t ne_max = (size_t)BQ_TREND_MAXP * (BQ_TREND_MAXP + 1);
    TrendPlan pl{};
    pl.nsl = npad / 64;
    pl.o_H = 0;
    pl.o_G = (size_t)BQ_TREND_ROWS * npad;
    pl.o_alpha = 2 * pl.o_G;
    pl.o_part = pl.o_alpha + (size_t)npad;
    pl.o_sums = pl.o_part + granule((size_t)pl.nsl * ne_max);
    pl.o_tr = pl.o_sums + granule(ne_max);
    pl.total = pl.o_tr + BQ_TREND_STATE;
    return pl;
}

// Without the variance there is no sweep; with it the p sums per point ride in the row reductions'
// one pass over V while a thread's registers hold them, and go out as a product from there on
TrendRoute trend_route(int p, bool want_var)
{
    if (!want_var)
        return TrendRoute::Mean;
    return p <= BQ_TREND_ONEPASS_MAXP ? TrendRoute::OnePass : TrendRoute::Gemm;
}

int launch_trend_basis(bq_ctx *c, int d, const double *x, int m, int mp, const TrendBasis &tb,
                       double *out, long rs, long cs)
{
    if (d < 1 || d > BQ_MAXD || m < 0 || mp < m || tb.p != trend_p(tb.degree, d) ||
        tb.p > BQ_TREND_MAXP)
        return fail(c, BQ_ERR_BAD_ARG, "trend: a basis of degree %d over %d of %d points", tb.degree,
                    m, mp);
    Bracket br(c, BQ_K_REDUCE, 8.0 * BQ_TREND_ROWS * mp);
    const dim3 grid((unsigned)((mp + 255) / 256));
    BQ_DISPATCH_D(d, hipLaunchKernelGGL(trend_basis_kernel<D>, grid, dim3(256), 0, c->stream, x, m, mp,
                                        tb, out, rs, cs));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_trend_sums(bq_ctx *c, const double *G, const double *z, int npad, int p, double *part,
                      double *sums)
{
    if (p < 1 || p > BQ_TREND_MAXP || npad <= 0 || (npad & 63))
        return fail(c, BQ_ERR_BAD_ARG, "trend: %d basis rows over %d columns", p, npad);
    const int ne = p * p + p, nsl = npad / 64;
    Bracket br(c, BQ_K_REDUCE, 8.0 * BQ_TREND_ROWS * npad);
    hipLaunchKernelGGL(trend_sums_kernel, dim3((unsigned)nsl), dim3(256), 0, c->stream, G, z, p, part);
    HIPCHK(c, hipGetLastError());
    launch_fold(c, part, nsl, ne, 1, ne, sums);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_trend_solve(bq_ctx *c, const double *sums, int p, const double *G, const double *z,
                       int npad, double *tr, double *zt)
{
    if (p < 1 || p > BQ_TREND_MAXP || npad <= 0)
        return fail(c, BQ_ERR_BAD_ARG, "trend: %d basis rows over %d columns", p, npad);
    Bracket br(c, BQ_K_POTF2, (double)p * p * p / 3.0);
    hipLaunchKernelGGL(trend_solve_kernel, dim3(1), dim3(256), 0, c->stream, sums, p, G, z, npad, tr,
                       zt);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_rowdot_trend(bq_ctx *c, const double *V, long ldv, int M, int Mp, int npad,
                        const double *z, double k0, const double *G, int p, double *mean,
                        double *var, double *R)
{
    if (p < 1 || p > BQ_TREND_ONEPASS_MAXP || M < 1 || Mp < M || (Mp & 15) || !z || !mean || !var)
        return fail(c, BQ_ERR_BAD_ARG, "trend: %d sums in one pass over %d rows", p, M);
    Bracket br(c, BQ_K_REDUCE);
#define BQ_ROWDOT_TREND(NB_)                                                                       \
    case NB_:                                                                                      \
        hipLaunchKernelGGL(rowdot_trend_kernel<NB_>, dim3(Mp / 16), dim3(1024), 0, c->stream, V,   \
                           ldv, M, npad, z, k0, G, mean, var, R, (long)Mp);                        \
        break
    switch (p) {
        BQ_ROWDOT_TREND(1);
        BQ_ROWDOT_TREND(2);
        BQ_ROWDOT_TREND(3);
        BQ_ROWDOT_TREND(4);
        BQ_ROWDOT_TREND(5);
        BQ_ROWDOT_TREND(6);
        BQ_ROWDOT_TREND(7);
        BQ_ROWDOT_TREND(8);
    }
#undef BQ_ROWDOT_TREND
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_trend_finish(bq_ctx *c, const double *R, long ldr, int M, int p, const double *tr,
                        double *mean, double *var, double *status)
{
    if (p < 1 || p > BQ_TREND_MAXP || M < 1)
        return fail(c, BQ_ERR_BAD_ARG, "trend: %d basis columns at %d points", p, M);
    Bracket br(c, BQ_K_REDUCE, 8.0 * (double)M * p);
    hipLaunchKernelGGL(trend_finish_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, c->stream,
                       R, ldr, M, p, tr, mean, var, status);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_trend_mean(bq_ctx *c, int d, const double *xo, int M, const double *pts, int n,
                      const double *alpha_t, const GaussParams &g, const TrendBasis &tb,
                      const double *tr, double *mean, double *status)
{
    if (d < 1 || d > BQ_MAXD || M < 1 || tb.p != trend_p(tb.degree, d))
        return fail(c, BQ_ERR_BAD_ARG, "trend: a basis of degree %d at %d points", tb.degree, M);
    Bracket br(c, BQ_K_REDUCE);
    dim3 grid((unsigned)((M + 3) / 4));
    BQ_DISPATCH_D(d, hipLaunchKernelGGL(trend_mean_kernel<D>, grid, dim3(256), 0, c->stream, xo, M,
                                        pts, n, alpha_t, g, tb, tr, mean, status));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_neg_identity(bq_ctx *c, double *nr, int B, int npad)
{
    hipLaunchKernelGGL(neg_identity_kernel, dim3((npad + 255) / 256), dim3(256), 0, c->stream, nr,
                       B, npad);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_pad_identity(bq_ctx *c, double *A, long lda, int n, int ntot)
{
    hipLaunchKernelGGL(pad_identity_kernel, dim3((ntot + 255) / 256, ntot), dim3(256), 0, c->stream,
                       A, lda, n, ntot);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// out = 2 sum log diag[i * (stride + 1)]
int launch_logdet(bq_ctx *c, const double *diag, long stride, int n, double *out)
{
    hipLaunchKernelGGL(logdet_kernel, dim3(1), dim3(256), 0, c->stream, diag, stride, n, out);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// dst (cols x rows, ld ldd) = src (rows x cols, ld lds)^T, 64 x 64 tiles
int launch_transpose_pad(bq_ctx *c, const double *src, long lds, int rows, int cols, double *dst,
                         long ldd)
{
    const dim3 g((rows + 63) / 64, (unsigned)((cols + 63) / 64));
    hipLaunchKernelGGL(transpose_pad_kernel, g, dim3(256), 0, c->stream, src, lds, rows, cols, dst,
                       ldd);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// dst block = src block^T for `batch` blocks of ld B, bx x by tiles of 64 each
int launch_transpose_blocks(bq_ctx *c, const double *src, double *dst, int B, long bstride,
                            int bx, int by, int batch)
{
    hipLaunchKernelGGL(transpose_blocks_kernel, dim3(bx, by, batch), dim3(256), 0, c->stream, src,
                       dst, B, bstride);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_neg_sumsq(bq_ctx *c, const double *v, int n, double *out)
{
    hipLaunchKernelGGL(neg_sumsq_kernel, dim3(1), dim3(256), 0, c->stream, v, n, out);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// ---- growing a resident fit (append.h; fit.hip, bq_gp_append) ----
size_t append_parts(int npad) { return (size_t)((npad + BQ_APPEND_CHUNK - 1) / BQ_APPEND_CHUNK); }
size_t append_part_doubles(int npad) { return append_parts(npad) * BQ_APPEND_PART; }

// k <= 64: the partial products over V's column chunks, then the one-workgroup factor of S
int launch_append_small(bq_ctx *c, const double *V, int npad, int k, const double *z, long zstride,
                        double *part, const double *xn, const double *yn, int d,
                        const GaussParams &g, double tol, double *S, double *zn,
                        int *info)
{
    if (k < 1 || k > 64 || npad <= 0 || (npad & 63))
        return fail(c, BQ_ERR_BAD_ARG, "append: 1 <= k <= 64 rows over whole 64-column blocks");
    const int np = (int)append_parts(npad);
    {
        Bracket br(c, BQ_K_REDUCE, 8.0 * 64 * npad);
        hipLaunchKernelGGL(append_part_kernel, dim3(np), dim3(256), 0, c->stream, V, npad, k, z,
                           zstride, part);
        HIPCHK(c, hipGetLastError());
    }
    Bracket br(c, BQ_K_POTF2, (double)k * k * k / 3.0);
    hipLaunchKernelGGL(append_factor_kernel, dim3(1), dim3(256), 0, c->stream, part, np, xn, yn, d,
                       k, g, tol, S, zn, info);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_append_rhs(bq_ctx *c, const double *yn, const double *vz, int k, double *X,
                      const double *S, int kp, double tol, int *info)
{
    hipLaunchKernelGGL(append_rhs_kernel, dim3(1), dim3(256), 0, c->stream, yn, vz, k, X, S, kp, tol,
                       info);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_append_commit(bq_ctx *c, const AppendJob &a)
{
    Bracket br(c, BQ_K_REDUCE, 16.0 * a.k * (a.n + a.k));
    const long words = (long)a.k * (a.n + a.k);
    const int wgs = (int)std::max(1L, std::min((long)c->cus, (words + 4095) / 4096));
    hipLaunchKernelGGL(append_commit_kernel, dim3(wgs), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_append_grow(bq_ctx *c, double *A, long lda, int r0, int ntot, int yrow,
                       const double *Aold, long ldold, int yold, int ncopy)
{
    if (r0 >= ntot)
        return BQ_OK;
    hipLaunchKernelGGL(append_grow_kernel, dim3((ntot - r0 + 255) / 256, ntot), dim3(256), 0,
                       c->stream, A, lda, r0, ntot, yrow, Aold, ldold, yold, ncopy);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// ---- shrinking a resident fit (remove.h; fit.hip, bq_gp_remove) ----
int launch_remove_compact(bq_ctx *c, const RemoveJob &r)
{
    Bracket br(c, BQ_K_REDUCE, 8.0 * r.ntot2 * (0.5 * r.npad2 + r.kp));
    const dim3 grid(r.ntot2 / 64, r.npad2 / 64 + 1 + r.kp / 64);
    hipLaunchKernelGGL(remove_compact_kernel, grid, dim3(256), 0, c->stream, r);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_remove_trail(bq_ctx *c, double *A, long ldl, int yrow, double *pts, double *y, int d,
                        int n2, int n, int npad)
{
    Bracket br(c, BQ_K_REDUCE, 8.0 * (n - n2) * npad);
    hipLaunchKernelGGL(remove_trail_kernel, dim3((npad + 255) / 256), dim3(256), 0, c->stream, A,
                       ldl, yrow, pts, y, d, n2, n, npad);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// block column J of one sweep: the diagonal launch, then the row blocks below it (nblocks = every
// 64-row block of the system, the border block included)
int launch_remove_step(bq_ctx *c, double *A, long lda, double *V, long ldv, int J, int nblocks,
                       double *Ms)
{
    constexpr size_t lds = sizeof(double) * BQ_REMOVE_LDS_DOUBLES;
    if (J < 0 || J + 1 >= nblocks)
        return fail(c, BQ_ERR_BAD_ARG, "remove: block column %d of %d", J, nblocks);
    if (!c->remove_lds_set) {
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(remove_diag_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        c->remove_lds_set = true;
    }
    {
        Bracket br(c, BQ_K_POTF2, 2.0 * 64 * 64 * 64);
        hipLaunchKernelGGL(remove_diag_kernel, dim3(1), dim3(256), lds, c->stream, A, lda, V, ldv, J,
                           Ms);
        HIPCHK(c, hipGetLastError());
    }
    const int below = nblocks - J - 1;
    Bracket br(c, BQ_K_GEMM, 2.0 * 64 * below * 128 * 128);
    hipLaunchKernelGGL(remove_rows_kernel, dim3(below), dim3(256), 0, c->stream, A, lda, V, ldv, J,
                       Ms);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_remove_finish(bq_ctx *c, const double *A, long lda, int yrow, int n, int npad,
                         double *dinv, double *out)
{
    Bracket br(c, BQ_K_REDUCE, 16.0 * npad);
    hipLaunchKernelGGL(remove_finish_kernel, dim3(1), dim3(256), 0, c->stream, A, lda, yrow, n, npad,
                       dinv, out);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// one B-column step of the forward single-vector sweep (trsv.h)
int launch_trsv_fwd(bq_ctx *c, const double *L, long ldl, int J, int bJ, int B, int nupd,
                    const double *nr, const double *tt, double *x, double *y, double work)
{
    Bracket br(c, BQ_K_GEMM, work);
#define BQ_TRSV_FWD(NB_)                                                                           \
    hipLaunchKernelGGL((trsv_fwd_step_kernel<NB_>), dim3(bJ / 16 + nupd), dim3(1024), 0, c->cur,  \
                       L, ldl, J, bJ, B, nr, tt, x, y)
    if (B == 512)
        BQ_TRSV_FWD(8);
    else if (B == 256)
        BQ_TRSV_FWD(4);
    else
        BQ_TRSV_FWD(0);
#undef BQ_TRSV_FWD
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_trsv_bwd(bq_ctx *c, const double *L, long ldl, int J, int bJ, int B, int bn, int nupd,
                    const double *nt, const double *uu, double *x, double *y, double work)
{
    Bracket br(c, BQ_K_GEMM, work);
    hipLaunchKernelGGL(trsv_bwd_step_kernel, dim3(bJ / 16 + nupd), dim3(1024), 0, c->cur, L, ldl, J,
                       bJ, B, bn, nt, uu, x, y);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// doubles of workspace a one-launch sweep needs behind its vectors: the ticket (one 64-byte
// line) and the x versions 1 .. ns - 1
size_t trsv_flow_ws_doubles(int npad, int B)
{
    const int ns = (npad + B - 1) / B;
    return 8 + (size_t)(ns > 1 ? ns - 1 : 0) * npad;
}

bool trsv_flow_ok(const bq_ctx *c, int npad, int B, bool prefilled)
{
    // (below 2048 rows the sweep is two to four steps: the memsets cost what the launches did --
    // unless the caller fills the slots on its way in, bq_gp_solve: then from 1024 rows, half the
    // threshold: n = 1000 0.061 -> 0.053 ms, 1536 0.077 -> 0.074)
    constexpr int kFlowMin = 2048;
    return c->cfg.trsv_flow && c->flow_abort && B <= 512 && (B & 63) == 0 && (npad & 63) == 0 &&
           npad >= (prefilled ? kFlowMin / 2 : kFlowMin) && (npad + B - 1) / B >= 2;
}

// ws: trsv_flow_ws_doubles(npad, B) doubles; x0 is read, y written (npad each)
int launch_flow_in(bq_ctx *c, const double *hsrc, int n, double *x, int npad, double *fill,
                   size_t nfill)
{
    const long blocks = std::min<long>(1024, (std::max<long>(npad, (long)nfill) + 255) / 256);
    hipLaunchKernelGGL(flow_in_kernel, dim3((unsigned)blocks), dim3(256), 0, c->cur, hsrc, n, x, npad,
                       reinterpret_cast<unsigned long long *>(fill), (long)nfill);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_copy_words2(bq_ctx *c, void *d1, const void *s1, size_t n1, void *d2, const void *s2,
                       size_t n2)
{
    hipLaunchKernelGGL(copy_words2_kernel, dim3(1), dim3(256), 0, c->cur,
                       static_cast<unsigned long long *>(d1),
                       static_cast<const unsigned long long *>(s1), (int)n1,
                       static_cast<unsigned long long *>(d2),
                       static_cast<const unsigned long long *>(s2), (int)n2);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_plan_scatter(bq_ctx *c, const double *stage, int nprob, int d, int n, int M, int ntot,
                        int npad, int gw, double *gp, double *pts, double *yd)
{
    const long total = (long)nprob * (gw + (long)d * n + (long)d * M + n);
    hipLaunchKernelGGL(plan_scatter_kernel, dim3((unsigned)std::min<long>(256, (total + 255) / 256)),
                       dim3(256), 0, c->cur, stage, nprob, d, n, M, ntot, npad, gw, gp, pts, yd);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_plan_gather(bq_ctx *c, double *out, const double *scal, const int *info,
                       const double *mean, const double *var, int nb, int M)
{
    const long total = std::max<long>(4L * nb, (long)M * nb);
    hipLaunchKernelGGL(plan_gather_kernel, dim3((unsigned)std::min<long>(64, (total + 255) / 256)),
                       dim3(256), 0, c->cur, out, scal, info, mean, var, nb, M);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_small_potrs(bq_ctx *c, double *stage, int n, int nrhs)
{
    hipLaunchKernelGGL(small_potrs_kernel, dim3(1), dim3(1024), 0, c->cur, stage, n, nrhs);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_mat_in(bq_ctx *c, const double *stage, int n, double *A, long lda, int ntot, int *info)
{
    const long total = (long)ntot * ntot;
    hipLaunchKernelGGL(mat_in_kernel, dim3((unsigned)std::min<long>(256, (total + 255) / 256)),
                       dim3(256), 0, c->cur, stage, n, A, lda, ntot, info);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_mat_out(bq_ctx *c, double *out, const double *A, long lda, int n, const int *info)
{
    const long total = (long)n * n;
    hipLaunchKernelGGL(mat_out_kernel, dim3((unsigned)std::min<long>(256, (total + 255) / 256)),
                       dim3(256), 0, c->cur, out, A, lda, n, info);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// the context's mapped pinned staging buffer, at least `words` doubles: host and device views
int ctx_stage(bq_ctx *c, size_t words, double **host, double **dev)
{
    if (c->hstage_len < words) {
        if (c->hstage)
            (void)hipHostFree(c->hstage);
        c->hstage = nullptr;
        c->hstage_len = 0;
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&c->hstage), sizeof(double) * words));
        c->hstage_len = words;
    }
    *host = c->hstage;
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(dev), c->hstage, 0));
    return BQ_OK;
}

int launch_gather_row(bq_ctx *c, double *dst, const double *src, long stride, int n)
{
    hipLaunchKernelGGL(gather_row_kernel, dim3((n + 255) / 256), dim3(256), 0, c->cur, dst, src,
                       stride, n);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_flow_out(bq_ctx *c, const double *x, int n, double *hdst)
{
    hipLaunchKernelGGL(flow_out_kernel, dim3((n + 255) / 256), dim3(256), 0, c->cur, x, n, hdst);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_trsv_flow(bq_ctx *c, bool forward, const double *L, long ldl, int npad, int B,
                     const double *m1, const double *m2, const double *x0, double *y, double *ws,
                     bool preset)
{
    const int ns = (npad + B - 1) / B, last = (npad - 1) / B * B;
    long blocks = 0;
    double work = 0.0;
    for (int s = 0; s < ns; ++s) {
        const int J = forward ? s * B : last - s * B;
        const int bJ = std::min(B, npad - J);
        const int nupd = forward ? (s > 0 ? (npad - J - bJ) / 64 : 0) : (s > 0 ? J / 64 : 0);
        blocks += bJ / 16 + nupd;
        work += (double)bJ * bJ + 2.0 * B * (bJ + 64.0 * nupd);
    }
    // every slot starts as the sentinel (all bits set); the ticket counter starts at -1 with it
    // (preset: the caller has filled ws and y already -- flow_in_kernel, both sweeps of a solve)
    if (!preset) {
        HIPCHK(c, hipMemsetAsync(ws, 0xFF, sizeof(double) * trsv_flow_ws_doubles(npad, B), c->cur));
        HIPCHK(c, hipMemsetAsync(y, 0xFF, sizeof(double) * (size_t)npad, c->cur));
    }
    // (BQ_FLOW_FAULT=1, read per launch: the forward sweep loses a hand-off -- tests of the time-out)
    const int fault = std::getenv("BQ_FLOW_FAULT") ? std::atoi(std::getenv("BQ_FLOW_FAULT")) : 0;
    Bracket br(c, BQ_K_GEMM, work);
    int *ticket = reinterpret_cast<int *>(ws);
    double *xv = ws + 8;
    if (!forward)
        hipLaunchKernelGGL(trsv_bwd_flow_kernel, dim3((unsigned)blocks), dim3(1024), 0, c->cur, L, ldl,
                           npad, B, m1, m2, x0, xv, y, ticket, c->flow_abort, fault);
    else if (B == 512)
        hipLaunchKernelGGL(trsv_fwd_flow_kernel<8>, dim3((unsigned)blocks), dim3(1024), 0, c->cur, L,
                           ldl, npad, B, m1, m2, x0, xv, y, ticket, c->flow_abort, fault);
    else if (B == 256)
        hipLaunchKernelGGL(trsv_fwd_flow_kernel<4>, dim3((unsigned)blocks), dim3(1024), 0, c->cur, L,
                           ldl, npad, B, m1, m2, x0, xv, y, ticket, c->flow_abort, fault);
    else
        hipLaunchKernelGGL(trsv_fwd_flow_kernel<0>, dim3((unsigned)blocks), dim3(1024), 0, c->cur, L,
                           ldl, npad, B, m1, m2, x0, xv, y, ticket, c->flow_abort, fault);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// reads and clears the abort word (call with the stream synchronised)
bool flow_timed_out(bq_ctx *c)
{
    if (c->flow_abort && *static_cast<volatile int *>(c->flow_abort) != 0) {
        *c->flow_abort = 0;
        return true;
    }
    return false;
}

// a time-out nobody handled (every entry point that launches a one-launch sweep re-issues the
// solve itself: with_flow_fallback): bq_ctx_sync reports it
int flow_check(bq_ctx *c)
{
    if (flow_timed_out(c))
        return fail(c, BQ_ERR_HIP, "single-vector sweep: a hand-off between workgroups timed out "
                                   "(BQ_TRSV_FLOW=0 selects the one-launch-per-block sweeps)");
    return BQ_OK;
}

} // namespace bqh
