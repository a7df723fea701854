// fit.hip -- device-resident GP fits (bq_fit): factor, z = L^-1 y, log-ML; alpha, the block
// inverses and the sweep workspaces on demand (gp.GP.Lxx / inv_Kxx_y / log_lh / mean / cov:
// bq.py:200,227-228,282,334-335,546,942-943).
#include "host.h"

// ===========================================================================
// GP fit objects
// ===========================================================================
namespace bqh {

// a fit's pinned staging (bq_fit::hfit): [0, 136) results, then the kernel parameters, then 64
// points of the largest dimension (the border points of a refit, the observations of an append)
constexpr size_t HF_PAR = 8 + 128, HF_PTS = HF_PAR + (sizeof(GaussParams) + 7) / 8;
constexpr size_t HF_NPTS = 64 * BQ_MAXD;

// the pinned staging of a fit, allocated on its first use
static int fit_stage(bq_ctx *c, bq_fit *f)
{
    if (!f->hfit)
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&f->hfit),
                                sizeof(double) * (HF_PTS + HF_NPTS)));
    return BQ_OK;
}

// new hyper-parameters, and a layout with M border points behind the fit's own
static void fit_set_params(bq_fit *f, double h, const double *w, double s, int M)
{
    f->h = h;
    f->s = s;
    for (int k = 0; k < f->d; ++k)
        f->w[k] = w[k];
    f->g = make_params(f->d, h, w, s);
    f->L = make_layout(f->n, M, true); // same ntot: border points share the y row's block
}

// A pinned staging buffer of a fit as both sides see it.  Its small transfers go through one kernel
// each on the device's view: a copy-engine operation costs the stream 8-9 us, a further kernel 2.9
// (tools/stream_ops_bench.hip); a refit at the reference's own sizes is 40 us in all.
struct Staging {
    double *host = nullptr;
    double *dev = nullptr; // null: kernel copies are off (BQ_SOLVE_KCOPY=0), the copy engine moves it
};

static int stage_view(bq_ctx *c, double *host, Staging &st)
{
    st.host = host;
    st.dev = nullptr;
    if (c->cfg.solve_kcopy && host)
        HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&st.dev), host, 0));
    return BQ_OK;
}

// n1 (and n2) 8-byte words between device memory p1 (p2) and the staging at word at1 (at2), `in`:
// towards the device: one launch, else a copy-engine operation each
static int stage_copy(bq_ctx *c, const Staging &st, bool in, void *p1, size_t at1, size_t n1,
                      void *p2 = nullptr, size_t at2 = 0, size_t n2 = 0)
{
    if (st.dev) {
        double *m1 = st.dev + at1, *m2 = n2 ? st.dev + at2 : nullptr;
        return in ? launch_copy_words2(c, p1, m1, n1, p2, m2, n2)
                  : launch_copy_words2(c, m1, p1, n1, m2, p2, n2);
    }
    const hipMemcpyKind kind = in ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    double *h1 = st.host + at1, *h2 = st.host + at2;
    HIPCHK(c, hipMemcpyAsync(in ? p1 : h1, in ? h1 : p1, sizeof(double) * n1, kind, c->stream));
    if (n2)
        HIPCHK(c, hipMemcpyAsync(in ? p2 : h2, in ? h2 : p2, sizeof(double) * n2, kind, c->stream));
    return BQ_OK;
}

// pm / pv: device buffers for the posterior mean / variance of the layout's M border points
// (bq_gp_refit_predict), or null
// npts_words: that many doubles of border points wait in the staging buffer (hfit + HF_PTS) for
// their place behind the fit's own points
static int fit_factor(bq_ctx *c, bq_fit *f, double *pm = nullptr, double *pv = nullptr,
                      double *hpost = nullptr, // hpost: host copy of misc[8 .. 8 + 128) on return
                      size_t npts_words = 0)
{
    int *info = f->misc.i();
    double *scal = f->misc.d() + 2;
    f->valid = false;
    f->stale = false;
    f->drop(bq_fit::FACTOR_CHANGED);
    BQCHK(fit_stage(c, f));
    std::memcpy(f->hfit + HF_PAR, &f->g, sizeof f->g);
    // the call's small transfers: kernel parameters (and border points) in, the record out
    Staging st;
    BQCHK(stage_view(c, f->hfit, st));
    static_assert(sizeof(GaussParams) % 8 == 0, "GaussParams is copied in 8-byte words");
    BQCHK(stage_copy(c, st, true, f->gp.p, HF_PAR, sizeof f->g / 8,
                     f->pts.d() + (size_t)f->d * f->npad, HF_PTS, npts_words));
    const GramSeed sys{f->pts.d(), 0, f->y.d(), 0, static_cast<const GaussParams *>(f->gp.p), 0,
                       f->L, f->d, 0, 0};
    BQCHK(enqueue_bordered(c, sys, 1, f->A.d(), f->ldl, 0, f->dinv.d() + f->npad, info,
                           f->panel.d(), f->panel.bytes / sizeof(double), scal, pm, pv, 64L, false,
                           0.0));
    // one read-back: misc = [info (int, 8 bytes) | pad | scal[4] | pad | mean[64] | var[64]]
    const double *hm = f->hfit;
    BQCHK(stage_copy(c, st, false, f->misc.p, 0, hpost ? 8 + 128 : 6));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hpost)
        std::memcpy(hpost, hm + 8, sizeof(double) * 128);
    int hinfo = 0;
    std::memcpy(&hinfo, hm, sizeof hinfo);
    const double *hs = hm + 2;
    if (hinfo != 0)
        return fail(c, BQ_ERR_NOT_PD, "matrix is not positive definite");
    f->logml = hs[0];
    f->logdet = hs[1];
    f->qf = hs[2];
    f->valid = true;
    return BQ_OK;
}

// every consumer of a fit: the handle exists and its last factorisation succeeded
int check_fit(bq_ctx *c, const bq_fit *f)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!f)
        return fail(c, BQ_ERR_BAD_ARG, "null fit handle");
    if (f->stale)
        return fail(c, BQ_ERR_BAD_ARG,
                    "fit has new targets (bq_gp_set_y): refit required before its next use");
    if (!f->valid)
        return fail(c, BQ_ERR_NOT_PD,
                    "fit holds no valid factor: its last (re)fit was not positive definite");
    return BQ_OK;
}

// the 16 x 16 block inverses of the resident factor's diagonal (the record trsm_blk_kernel
// wants), built on their first use after a (re)fit
int fit_dw(bq_ctx *c, bq_fit *f)
{
    if (!(f->have & bq_fit::DW)) {
        BQCHK(launch_diag_winv(c, f->A.d(), f->ldl, f->npad, f->dw.d()));
        f->have |= bq_fit::DW;
    }
    return BQ_OK;
}

// the wide block inverses of the resident factor, built on the first sweep after a (re)fit: a
// hyper-parameter loop that only reads log-ML never pays for them
int fit_wide(bq_ctx *c, bq_fit *f, WideInv &w)
{
    if (!(f->have & bq_fit::WIDE)) {
        BQCHK(fit_dw(c, f));
        BQCHK(fit_grow(c, f->wide, sizeof(double) * wide_alloc_doubles(f->npad),
                       "wide block inverses"));
        BQCHK(compute_wide_inverses(c, f->A.d(), f->ldl, f->npad, f->dw.d(), f->wide.d()));
        f->have |= bq_fit::WIDE;
    }
    w = wide_views(f->wide.d(), f->npad);
    return BQ_OK;
}

// the single-vector workspace of a fit (x at vec, y at vec + npad)
int fit_vec(bq_ctx *c, bq_fit *f)
{
    // x | y | the one-launch sweeps' workspace (ticket + x versions) | a solve's second vector
    // and second workspace (bq_gp_solve: both sweeps' slots are filled in one launch)
    const size_t need = 3 * (size_t)f->npad + 2 * trsv_flow_ws_doubles(f->npad, wide_block(f->npad));
    BQCHK(fit_grow(c, f->vec, sizeof(double) * need, "single-vector workspace"));
    if (!f->hvec)
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&f->hvec),
                                sizeof(double) * (size_t)f->npad));
    return BQ_OK;
}

int fit_alpha(bq_ctx *c, bq_fit *f)
{
    if (f->have & bq_fit::ALPHA)
        return BQ_OK;
    // alpha = L^-T z, z = A[yrow, 0:npad] (the forward-solved y of the bordered system)
    WideInv w;
    BQCHK(fit_wide(c, f, w));
    BQCHK(fit_vec(c, f));
    // (the gather stays outside the captured chain: the y row moves when the fit carries
    // border points, bq_gp_refit_predict)
    BQCHK(with_flow_fallback(c, [&]() -> int {
        BQCHK(launch_gather_row(c, f->vec.d(), f->A.d() + f->L.yrow, f->ldl, f->npad));
        BQCHK(fit_replay(c, f, 1, [&]() -> int {
            return enqueue_backward_vec(c, f->vec.d(), f->alpha.d(), f->A.d(), f->ldl, f->npad, w,
                                        f->vec.d() + 2 * (size_t)f->npad);
        }));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BQ_OK;
    }));
    f->have |= bq_fit::ALPHA;
    return BQ_OK;
}

} // namespace bqh

using namespace bqh;

extern "C" int bq_gp_fit(bq_ctx *c, const double *x, const double *y, int64_t d, int64_t n,
                         double h, const double *w, double s, bq_fit **out)
{
    if (!out)
        return BQ_ERR_BAD_ARG;
    *out = nullptr;
    BQCHK(check_dims(c, d, n));
    BQCHK(check_w(c, d, h, w, s));
    if (!x || !y)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    bq_fit *f = new (std::nothrow) bq_fit();
    if (!f)
        return fail(c, BQ_ERR_NOMEM, "out of host memory");
    f->d = (int)d;
    f->n = (int)n;
    fit_set_params(f, h, w, s, 0);
    int st = f->alloc(c, (int)d, (int)n, "fit allocation failed");
    if (st == BQ_OK) {
        hipError_t e = f->gp.alloc(sizeof(GaussParams));
        if (e == hipSuccess)
            e = f->misc.alloc(sizeof(double) * (8 + 128));
        if (e != hipSuccess)
            st = fail(c, e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP,
                      "fit allocation failed: %s", hipGetErrorString(e));
    }
    if (st != BQ_OK) {
        delete f;
        return st;
    }
    auto H = [&](hipError_t err) {
        if (st == BQ_OK && err != hipSuccess)
            st = fail(c, BQ_ERR_HIP, "fit upload failed: %s", hipGetErrorString(err));
    };
    H(hipMemsetAsync(f->pts.p, 0, f->pts.bytes, c->stream));
    H(hipMemsetAsync(f->y.p, 0, f->y.bytes, c->stream));
    H(hipMemcpyAsync(f->pts.p, x, sizeof(double) * d * n, hipMemcpyHostToDevice, c->stream));
    H(hipMemcpyAsync(f->y.p, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (st == BQ_OK)
        st = fit_factor(c, f);
    if (st != BQ_OK) {
        (void)hipStreamSynchronize(c->stream);
        delete f;
        return st;
    }
    *out = f;
    return BQ_OK;
}

extern "C" int bq_gp_refit(bq_ctx *c, bq_fit *f, double h, const double *w, double s)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!f)
        return fail(c, BQ_ERR_BAD_ARG, "null fit handle");
    BQCHK(check_w(c, f->d, h, w, s));
    HIPCHK(c, hipSetDevice(c->device));
    fit_set_params(f, h, w, s, 0);
    return fit_factor(c, f);
}

// New targets for the same points: the hyper-parameter loop hands GP2 new targets l_sc =
// [l_s, exp(mean of GP1 at the candidates)] on every evaluation (bq.py:948-954) -- a new fit
// object per evaluation costs 0.10 ms at the reference's sizes and 0.57 ms at N = 1034, a
// refit 0.05 / 0.32.  Until its next bq_gp_refit / bq_gp_refit_predict every consumer of the
// fit returns BQ_ERR_BAD_ARG ("refit required") -- not BQ_ERR_NOT_PD: nothing failed.
extern "C" int bq_gp_set_y(bq_ctx *c, bq_fit *f, const double *y)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!f)
        return fail(c, BQ_ERR_BAD_ARG, "null fit handle");
    if (!y)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    f->stale = true; // the factor is intact, z / alpha / log-ML belong to the old targets
    f->drop(bq_fit::TARGETS_CHANGED);
    HIPCHK(c, hipMemcpyAsync(f->y.p, y, sizeof(double) * f->n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // y is the caller's buffer
    return BQ_OK;
}

// New hyper-parameters AND the posterior at M points in the same sweep -- the body of the
// hyper-parameter loop (bq.py:933-947: refit GP1, re-predict the candidates' mean and
// variance).  The M points ride as border rows of the fit's own bordered system, in the
// 64-row block that holds the y row anyway: no launch beyond the refit's, where a separate
// bq_gp_predict after a refit first rebuilds the factor's block inverses (N = 1024: 0.75 ms
// for refit + predict, 0.31 for this).  M <= 63; more points take the two-call route.
extern "C" int bq_gp_refit_predict(bq_ctx *c, bq_fit *f, double h, const double *w, double s,
                                   const double *xo, int64_t M, double *mean, double *var)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!f)
        return fail(c, BQ_ERR_BAD_ARG, "null fit handle");
    if (M < 0 || (M > 0 && (!xo || (!mean && !var))))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (M == 0)
        return bq_gp_refit(c, f, h, w, s);
    if (M > 63) {
        BQCHK(bq_gp_refit(c, f, h, w, s));
        return bq_gp_predict(c, f, xo, M, mean, var, nullptr);
    }
    BQCHK(check_w(c, f->d, h, w, s));
    HIPCHK(c, hipSetDevice(c->device));
    fit_set_params(f, h, w, s, (int)M);
    BQCHK(fit_stage(c, f));
    std::memcpy(f->hfit + HF_PTS, xo, sizeof(double) * f->d * M);
    double hv[128];
    BQCHK(fit_factor(c, f, f->misc.d() + 8, f->misc.d() + 8 + 64, hv, (size_t)f->d * (size_t)M));
    for (int64_t i = 0; i < M; ++i) {
        if (mean)
            mean[i] = hv[i];
        if (var)
            var[i] = hv[64 + i];
    }
    return BQ_OK;
}

// Append k observations to a resident fit under its current hyper-parameters: O(k n^2), no Gram
// of the old points, no refactorisation (append.h has the arithmetic).  V, S, L_S and z_new live in
// the context's scratch; a grown layout is built in buffers of its own beside the old one.  The
// fit is touched by the last kernel alone, and only when every pivot of S was positive: a failed
// append -- not positive definite, out of memory -- leaves the handle exactly as it was.
extern "C" int bq_gp_append(bq_ctx *c, bq_fit *f, const double *x_new, const double *y_new,
                            int64_t k64)
{
    BQCHK(check_fit(c, f));
    if (!x_new || !y_new || k64 < 1)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    BQCHK(check_dims(c, f->d, (int64_t)f->n + k64));
    const int d = f->d, n = f->n, k = (int)k64, npad = f->npad;
    for (int64_t i = 0; i < (int64_t)d * k; ++i)
        if (!std::isfinite(x_new[i]))
            return fail(c, BQ_ERR_BAD_ARG, "append: points must be finite");
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(y_new[i]))
            return fail(c, BQ_ERR_BAD_ARG, "append: targets must be finite");
    HIPCHK(c, hipSetDevice(c->device));
    const int kp = (int)roundup(k, 64);
    const bool small = k <= 64;

    // ---- a layout that holds n + k points, in buffers of its own until the append has succeeded
    const bool grow = n + k > npad;
    FitCore grown;
    if (grow)
        BQCHK(grown.alloc(c, d, n + k, "append: growing the fit to %d points failed", n + k));
    FitCore &to = grow ? grown : *f; // where the commit writes

    // ---- side buffers
    Scratch sc(c);
    const size_t oV = sc.take((size_t)kp * npad), oS = sc.take((size_t)kp * kp),
                 oX = sc.take((size_t)64 * kp), ox = sc.take((size_t)d * k), oy = sc.take((size_t)k),
                 oout = sc.take(8), oinfo = sc.take(8),
                 opart = sc.take(small ? append_part_doubles(npad) : 0),
                 odw = sc.take(small ? 0 : BQ_DINV_HALF * (size_t)(kp / 64)),
                 ovz = sc.take(small ? 0 : (size_t)kp);
    BQCHK(sc.commit());
    double *V = sc.at(oV), *S = sc.at(oS), *X = sc.at(oX), *xn = sc.at(ox), *yn = sc.at(oy),
           *out = sc.at(oout);
    int *info = reinterpret_cast<int *>(sc.at(oinfo));

    // ---- the observations in: through the fit's mapped staging when they fit in it
    Staging st;
    BQCHK(stage_view(c, f->hfit, st));
    const size_t nx = (size_t)d * k;
    if (st.dev && nx + k <= HF_NPTS) {
        std::memcpy(f->hfit + HF_PTS, x_new, sizeof(double) * nx);
        std::memcpy(f->hfit + HF_PTS + nx, y_new, sizeof(double) * k);
        BQCHK(stage_copy(c, st, true, xn, HF_PTS, nx, yn, HF_PTS + nx, (size_t)k));
    } else {
        HIPCHK(c, hipMemcpyAsync(xn, x_new, sizeof(double) * nx, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(yn, y_new, sizeof(double) * k, hipMemcpyHostToDevice, c->stream));
    }

    // ---- V = K(x_new, x_old) L^-T: the 64-column sweep with the 16 x 16 inverses, in place (S
    // cancels when a new point lies near old ones: enqueue_forward_rows_blk says what the wide
    // inverses lose there).  Columns n .. npad of V stay zero: the padding is the identity.
    BQCHK(launch_gram_cross_pad(c, d, xn, k, kp, f->pts.d(), n, npad, f->g, V, kp));
    BQCHK(fit_dw(c, f));
    BQCHK(enqueue_forward_rows_blk(c, V, kp, kp, f->A.d(), f->ldl, npad, f->dw.d()));
    const double *zold = f->A.d() + f->L.yrow;

    // ---- L_S and z_new.  A pivot counts as positive above the factorisation's own backward error
    // (append.h, append_factor_kernel)
    const double tol = 4.0 * (n + k + 1.0) * std::numeric_limits<double>::epsilon() *
                       (f->g.c + f->g.s2);
    long zstride = 1;
    if (small) {
        BQCHK(launch_append_small(c, V, npad, k, zold, f->ldl, sc.at(opart), xn, yn, d, f->g, tol, S,
                                  X, info));
    } else {
        // S = K(x_new, x_new) + s^2 I (identity on its padding) - V V^T, the device Cholesky,
        // then one more 64-column sweep for z_new = L_S^-1 (y_new - V z) as row 0 of X
        double *vz = sc.at(ovz), *dwS = sc.at(odw);
        BQCHK(launch_gram_sym(c, d, xn, 0, static_cast<GaussParams *>(f->gp.p), 0, S, kp, 0, k, 1));
        if (kp > k)
            BQCHK(launch_pad_identity(c, S, kp, k, kp));
        GemmJob vvt;
        vvt.C = S, vvt.ldc = kp;
        vvt.P = V, vvt.ldp = kp;
        vvt.Q = V, vvt.qsj = 1, vvt.qsk = kp;
        vvt.m = kp, vvt.n = kp, vvt.k = npad;
        BQCHK(launch_gemm(c, BQ_K_GEMM, vvt));
        if (!c->dinv64.p)
            HIPCHK(c, c->dinv64.alloc(BQ_DINV_STRIDE * sizeof(double)));
        HIPCHK(c, hipMemsetAsync(info, 0, sizeof(int), c->stream));
        BQCHK(potrf_one(c, S, kp, kp, c->dinv64.d(), info));
        BQCHK(launch_rowdot(c, V, (long)kp, k, kp, npad, zold, 0.0, vz, nullptr, f->ldl));
        HIPCHK(c, hipMemsetAsync(X, 0, sizeof(double) * (size_t)64 * kp, c->stream));
        BQCHK(launch_append_rhs(c, yn, vz, k, X, S, kp, tol, info));
        BQCHK(launch_diag_winv(c, S, kp, kp, dwS));
        BQCHK(enqueue_forward_rows_blk(c, X, 64, 64, S, kp, kp, dwS));
        zstride = 64;
    }

    // ---- the grown layout: the old factor and its z, the identity on the new padding
    if (grow) {
        HIPCHK(c, hipMemcpy2DAsync(to.A.p, sizeof(double) * to.ldl, f->A.p,
                                   sizeof(double) * f->ldl, sizeof(double) * npad, npad,
                                   hipMemcpyDeviceToDevice, c->stream));
        BQCHK(launch_append_grow(c, to.A.d(), to.ldl, npad, to.L.ntot, to.L.yrow, f->A.d(), f->ldl,
                                 f->L.yrow, npad));
        HIPCHK(c, hipMemsetAsync(to.pts.p, 0, to.pts.bytes, c->stream));
        HIPCHK(c, hipMemsetAsync(to.y.p, 0, to.y.bytes, c->stream));
        HIPCHK(c, hipMemsetAsync(to.dinv.p, 0, to.dinv.bytes, c->stream));
        HIPCHK(c, hipMemcpyAsync(to.pts.p, f->pts.p, sizeof(double) * (size_t)d * n,
                                 hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(to.y.p, f->y.p, sizeof(double) * n, hipMemcpyDeviceToDevice,
                                 c->stream));
        HIPCHK(c, hipMemcpyAsync(to.dinv.p, f->dinv.p, sizeof(double) * npad,
                                 hipMemcpyDeviceToDevice, c->stream));
    }

    // ---- the commit: the only launch that writes into the fit
    AppendJob job{};
    job.V = V, job.S = S, job.zn = X, job.zstride = zstride, job.xn = xn, job.yn = yn;
    job.info = info;
    job.A = to.A.d(), job.ldl = to.ldl, job.pts = to.pts.d(), job.y = to.y.d();
    job.dinv = to.dinv.d();
    job.out = out;
    job.logdet = f->logdet, job.qf = f->qf;
    job.d = d, job.n = n, job.k = k, job.kp = kp, job.yrow = to.L.yrow;
    BQCHK(launch_append_commit(c, job));
    const double *hm = f->hfit;
    BQCHK(stage_copy(c, st, false, out, 0, 6));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int hinfo = 0;
    std::memcpy(&hinfo, hm, sizeof hinfo);
    if (hinfo != 0)
        return fail(c, BQ_ERR_NOT_PD,
                    "append: the Schur complement of the new points is not positive definite");

    // ---- bookkeeping: a fit of n + k points in every respect
    if (grow)
        fit_adopt(f, grown);
    f->n = n + k;
    f->L.n = n + k;
    f->drop(bq_fit::FACTOR_CHANGED);
    f->logml = hm[2];
    f->logdet = hm[3];
    f->qf = hm[4];
    return BQ_OK;
}

// Remove k observations from a resident fit under its current hyper-parameters: O(k n^2), no Gram,
// no refactorisation (remove.h has the arithmetic).  Decided once, here:
//   trailing   the removed are exactly the last k: no arithmetic on the factor -- in place when the
//              layout stays (identity back on the new padding), else the compaction alone;
//   update     everything else: one compaction into buffers of the new layout, then one sweep per 64
//              removed indices (highest first) from the block column of the sweep's first index.
// Every buffer is allocated before the first launch and the fit's own buffers are only read until
// the new ones are swapped in: a failed call leaves the handle exactly as it was.
extern "C" int bq_gp_remove(bq_ctx *c, bq_fit *f, const int64_t *idx, int64_t k64)
{
    BQCHK(check_fit(c, f));
    if (!idx || k64 < 1 || k64 >= f->n)
        return fail(c, BQ_ERR_BAD_ARG, "remove: 1 <= k < n indices");
    const int d = f->d, n = f->n, k = (int)k64, n2 = n - k;
    std::vector<int> rem, keep;
    try {
        rem.resize(k);
        keep.resize(n2);
    } catch (const std::bad_alloc &) {
        return fail(c, BQ_ERR_NOMEM, "out of host memory");
    }
    for (int j = 0; j < k; ++j) {
        if (idx[j] < 0 || idx[j] >= n)
            return fail(c, BQ_ERR_BAD_ARG, "remove: index %lld out of range [0, %d)",
                        (long long)idx[j], n);
        rem[j] = (int)idx[j];
    }
    std::sort(rem.begin(), rem.end());
    for (int j = 1; j < k; ++j)
        if (rem[j] == rem[j - 1])
            return fail(c, BQ_ERR_BAD_ARG, "remove: index %d given twice", rem[j]);
    for (int i = 0, j = 0, o = 0; i < n; ++i) {
        if (j < k && rem[j] == i)
            ++j;
        else
            keep[o++] = i;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const Layout L2 = make_layout(n2, 0, true);
    const bool trailing = rem[0] == n2;
    const bool inplace = trailing && L2.npad == f->npad && f->L.M == 0;
    const int kp = trailing ? 0 : (int)roundup(k, 64);

    // ---- buffers of the new layout, and the side buffers
    FitCore next; // (its layout is L2)
    if (!inplace)
        BQCHK(next.alloc(c, d, n2, "remove: the layout of %d points could not be allocated", n2));
    Scratch sc(c);
    const size_t oout = sc.take(8), oV = sc.take(inplace ? 0 : (size_t)L2.ntot * kp),
                 oM = sc.take(kp ? BQ_REMOVE_M_DOUBLES : 0),
                 okeep = sc.take(inplace ? 0 : ((size_t)n2 + 1) / 2),
                 orem = sc.take(kp ? ((size_t)k + 1) / 2 : 0);
    BQCHK(sc.commit());
    double *out = sc.at(oout);

    if (inplace) {
        BQCHK(launch_remove_trail(c, f->A.d(), f->ldl, f->L.yrow, f->pts.d(), f->y.d(), d, n2, n,
                                  f->npad));
        BQCHK(launch_remove_finish(c, f->A.d(), f->ldl, f->L.yrow, n2, f->npad, f->dinv.d(), out));
    } else {
        int *dkeep = reinterpret_cast<int *>(sc.at(okeep)), *drem = reinterpret_cast<int *>(sc.at(orem));
        HIPCHK(c, hipMemcpyAsync(dkeep, keep.data(), sizeof(int) * n2, hipMemcpyHostToDevice,
                                 c->stream));
        if (kp)
            HIPCHK(c, hipMemcpyAsync(drem, rem.data(), sizeof(int) * k, hipMemcpyHostToDevice,
                                     c->stream));
        RemoveJob job{};
        job.A = f->A.d(), job.ldl = f->ldl, job.yrow = f->L.yrow;
        job.pts = f->pts.d(), job.y = f->y.d();
        job.keep = dkeep, job.rem = drem;
        job.A2 = next.A.d(), job.ldl2 = next.ldl, job.pts2 = next.pts.d(), job.y2 = next.y.d();
        job.V = sc.at(oV);
        job.d = d, job.n2 = n2, job.npad2 = L2.npad, job.ntot2 = L2.ntot, job.k = k, job.kp = kp;
        BQCHK(launch_remove_compact(c, job));
        // sweep s takes the removed indices 64 s .. 64 s + 63 (ascending): rem[64 s] - 64 s
        // survivors lie ahead of its first one, and V's columns are zero above that row
        for (int s = kp / 64 - 1; s >= 0; --s) {
            const int first = rem[64 * s] - 64 * s;
            if (first >= n2)
                continue; // (every survivor lies ahead of this sweep's indices: its V is zero)
            for (int J = first / 64; J < L2.npad / 64; ++J)
                BQCHK(launch_remove_step(c, next.A.d(), next.ldl, job.V + (size_t)64 * s * L2.ntot,
                                         L2.ntot, J, L2.ntot / 64, sc.at(oM)));
        }
        BQCHK(launch_remove_finish(c, next.A.d(), next.ldl, L2.yrow, n2, L2.npad, next.dinv.d(),
                                   out));
    }
    double hout[6];
    HIPCHK(c, hipMemcpyAsync(hout, out, sizeof hout, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));

    // ---- bookkeeping: a fit of n - k points in every respect
    if (!inplace)
        fit_adopt(f, next);
    f->n = n2;
    f->L.n = n2;
    f->drop(bq_fit::FACTOR_CHANGED);
    f->logml = hout[2];
    f->logdet = hout[3];
    f->qf = hout[4];
    return BQ_OK;
}

extern "C" void bq_fit_destroy(bq_ctx *c, bq_fit *f)
{
    if (!f)
        return;
    if (c) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    delete f;
}

extern "C" int bq_gp_logml(bq_ctx *c, bq_fit *f, double *out)
{
    BQCHK(check_fit(c, f));
    if (!out)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    *out = f->logml;
    return BQ_OK;
}

// Y = L^-T in gY (the gradient's and the Hessian's operand), built on its first use after a (re)fit
static int fit_y(bq_ctx *c, bq_fit *f)
{
    if (f->have & bq_fit::Y)
        return BQ_OK;
    const int npad = f->npad;
    WideInv w;
    BQCHK(fit_wide(c, f, w));
    const size_t bytes = sizeof(double) * (size_t)npad * npad;
    if (f->gY.bytes < bytes || f->gX.bytes < bytes) {
        // both buffers or neither: a failed allocation leaves no half-made workspace for the
        // next call to run on.  The sweep never writes Y's strict lower triangle and the
        // product reads it in diagonal tiles: cleared once, here
        hipError_t e = f->gY.alloc(bytes);
        if (e == hipSuccess)
            e = f->gX.alloc(bytes);
        if (e == hipSuccess)
            e = hipMemsetAsync(f->gY.p, 0, bytes, c->stream);
        if (e != hipSuccess) {
            f->gY.release();
            f->gX.release();
            return fail(c, e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP,
                        "gradient workspace (2 x %zu bytes): %s", bytes, hipGetErrorString(e));
        }
    }
    BQCHK(enqueue_inverse_rows(c, f->gX.d(), f->gY.d(), f->A.d(), f->ldl, npad, w));
    f->have |= bq_fit::Y;
    return BQ_OK;
}

// d log p / d theta = 1/2 sum_ij G_ij dKxx_ij / d theta, G = alpha alpha^T - Kxx^-1, with
// Kxx^-1 = Y Y^T, Y = L^-T: the triangular inverse by the forward row sweep on I (kept until the
// next (re)fit), then one MFMA product over the lower tiles of Y Y^T seeded with alpha alpha^T whose
// tiles are reduced against the kernel's derivatives instead of stored (gemm_lds_grad_kernel)
extern "C" int bq_gp_logml_grad(bq_ctx *c, bq_fit *f, double *grad)
{
    BQCHK(check_fit(c, f));
    if (!grad)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d, npad = f->npad;
    BQCHK(fit_alpha(c, f));
    BQCHK(fit_y(c, f));
    const size_t np = grad_parts(npad, d);
    BQCHK(fit_grow(c, f->gpart, sizeof(double) * (np + BQ_MAXD + 2), "gradient partial sums"));
    GradJob gj;
    gj.alpha = f->alpha.d();
    gj.pts = f->pts.d();
    gj.part = f->gpart.d();
    gj.g = f->g;
    gj.n = f->n;
    GradScale sc{};
    sc.f[0] = 1.0 / f->h;
    for (int k = 0; k < d; ++k)
        sc.f[1 + k] = 0.5 / f->w[k];
    sc.f[d + 1] = f->s;
    double *gd = f->gpart.d() + np;
    BQCHK(launch_logml_grad(c, d, f->gY.d(), npad, gj, sc, gd));
    HIPCHK(c, hipMemcpyAsync(grad, gd, sizeof(double) * (d + 2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// the Hessian's workspace beside Kxx^-1 (hess_ws_doubles), kept with the fit
static int fit_hess_ws(bq_ctx *c, bq_fit *f)
{
    return fit_grow(c, f->hB, sizeof(double) * hess_ws_doubles(f->npad, f->d), "Hessian workspace");
}

static HessJob fit_hess_job(const bq_fit *f)
{
    HessJob hj;
    hj.pts = f->pts.d();
    hj.alpha = f->alpha.d();
    hj.g = f->g;
    for (int k = 0; k < BQ_MAXD; ++k)
        hj.iw[k] = k < f->d ? 1.0 / f->w[k] : 0.0;
    hj.n = f->n;
    hj.npad = f->npad;
    return hj;
}

// The Hessian's products stage in gX and hB (Kxx^-1, the d products Kxx^-1 dK/dw_k, the vectors
// D_p a and Kxx^-1 D_p a), built on its first use after a (re)fit or new targets: the Hessian's sums
// and both cross-validation gradients read it
static int fit_prod(bq_ctx *c, bq_fit *f)
{
    if (f->have & bq_fit::PROD)
        return BQ_OK;
    BQCHK(fit_hess_ws(c, f));
    BQCHK(fit_alpha(c, f));
    BQCHK(fit_y(c, f));
    BQCHK(launch_hess_products(c, f->d, f->gY.d(), f->gX.d(), f->hB.d(), fit_hess_job(f), f->y.d(),
                               f->h, f->s));
    f->have |= bq_fit::PROD;
    return BQ_OK;
}

namespace bqh {
// u = Kxx^-1 alpha and z_k = Kxx^-1 (D_k alpha), k < d, as rows 0 .. d of the 64 x npad matrix in
// dkz (ld 64; its other rows and its columns at or beyond n are zero), built on their first use
// after a (re)fit or new targets: the right-hand sides [alpha, D_1 alpha ..] by ptheta_dka_kernel,
// then the forward and the backward row sweep with 64 rows, as bq_gp_predict runs them for one
// point -- first half -> second half -> first half.
int fit_dkz(bq_ctx *c, bq_fit *f)
{
    if (f->have & bq_fit::DKZ)
        return BQ_OK;
    BQCHK(fit_alpha(c, f));
    WideInv w;
    BQCHK(fit_wide(c, f, w));
    const size_t half = (size_t)BQ_PTHETA_ROWS * f->npad;
    BQCHK(fit_grow(c, f->dkz, sizeof(double) * 2 * half, "hyper-parameter derivative workspace"));
    double *R = f->dkz.d(), *X = R + half;
    BQCHK(launch_ptheta_dka(c, f->d, fit_hess_job(f), R));
    BQCHK(enqueue_forward_rows(c, R, X, BQ_PTHETA_ROWS, BQ_PTHETA_ROWS, f->A.d(), f->ldl, f->npad, w));
    BQCHK(enqueue_backward_rows(c, X, R, BQ_PTHETA_ROWS, BQ_PTHETA_ROWS, f->A.d(), f->ldl, f->npad, w));
    f->have |= bq_fit::DKZ;
    return BQ_OK;
}
} // namespace bqh

// d^2 log p / d theta^2 in the gradient's parameter order (hess.h has the formula): the products
// stage (fit_prod: Kxx^-1 = Y Y^T into the sweep's idle workspace, one MFMA product Kxx^-1 dK/dw_k
// per length scale with the derivative generated from the points), then tile sums and the quadratic
// terms on the device; the (d + 2)^2 entries are put together here from those sums.  Kept until the
// fit changes.
extern "C" int bq_gp_logml_hess(bq_ctx *c, bq_fit *f, double *hess)
{
    BQCHK(check_fit(c, f));
    if (!hess)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d, np = d + 2;
    if (!(f->have & bq_fit::HESS)) {
        BQCHK(fit_prod(c, f));
        const double *sums = nullptr;
        BQCHK(launch_hess_sums(c, d, f->gX.d(), f->hB.d(), fit_hess_job(f), &sums));
        const int ng = hess_ng(d), nt = hess_nt(d), nq = hess_nq(d);
        double hs[hess_ng(BQ_MAXD) + hess_nt(BQ_MAXD) + hess_nq(BQ_MAXD)];
        HIPCHK(c, hipMemcpyAsync(hs, sums, sizeof(double) * (ng + nt + nq), hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const double *G = hs, *T = hs + ng, *Q = hs + ng + nt;
        const double h = f->h, s = f->s;
        double *H = f->hess;
        // 1/2 sum(G o D_pq) + 1/2 tr(Ki D_p Ki D_q), upper triangle
        for (int i = 0; i < np * np; ++i)
            H[i] = 0.0;
        H[0] = G[0] / (h * h) + 2.0 * T[0] / (h * h);
        H[np - 1] = 2.0 * s * T[1] / h;
        H[(np - 1) * np + np - 1] = G[ng - 1] + 2.0 * (s * s) * T[2];
        for (int k = 0; k < d; ++k) {
            H[1 + k] = G[1 + k] / h + T[3 + k] / h;
            H[(1 + k) * np + np - 1] = s * T[3 + d + k];
            for (int l = k; l < d; ++l)
                H[(1 + k) * np + 1 + l] =
                    0.5 * G[1 + d + hess_pair(d, k, l)] + 0.5 * T[3 + 2 * d + hess_pair(d, k, l)];
        }
        // - (D_p a)^T Ki (D_q a), and the mirror
        for (int p = 0, o = 0; p < np; ++p)
            for (int q = p; q < np; ++q, ++o) {
                H[p * np + q] -= Q[o];
                H[q * np + p] = H[p * np + q];
            }
        f->have |= bq_fit::HESS;
    }
    for (int i = 0; i < np * np; ++i)
        hess[i] = f->hess[i];
    return BQ_OK;
}

// the leave-one-out workspace (loo_ws_doubles), kept with the fit
static int fit_loo_ws(bq_ctx *c, bq_fit *f)
{
    return fit_grow(c, f->loo, sizeof(double) * loo_ws_doubles(f->npad, f->d),
                    "leave-one-out workspace");
}

// mu | var | lp on the device (npad apart behind k, q and the t_k) and L_loo in the handle
static int fit_loo(bq_ctx *c, bq_fit *f)
{
    if (f->have & bq_fit::LOO)
        return BQ_OK;
    BQCHK(fit_loo_ws(c, f));
    BQCHK(fit_alpha(c, f));
    BQCHK(fit_y(c, f));
    const double *vecs = nullptr, *total = nullptr;
    BQCHK(launch_loo(c, f->d, f->gY.d(), f->alpha.d(), f->y.d(), f->n, f->npad, f->loo.d(), &vecs,
                     &total));
    HIPCHK(c, hipMemcpyAsync(&f->loo_total, total, sizeof(double), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    f->have |= bq_fit::LOO;
    return BQ_OK;
}

// Leave-one-out cross-validation (loo.h has the formulas): the predictive mean, variance and log
// density of every observation from the n - 1 others, and their sum, from diag Kxx^-1 -- the row
// sums of squares of Y = L^-T -- and alpha.  Kept until the fit changes.
extern "C" int bq_gp_loo(bq_ctx *c, bq_fit *f, double *mean, double *var, double *logpred,
                         double *total)
{
    BQCHK(check_fit(c, f));
    if (!mean && !var && !logpred && !total)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    BQCHK(fit_loo(c, f));
    const double *vecs = f->loo.d() + (size_t)(f->d + 2) * f->npad;
    double *outs[3] = {mean, var, logpred};
    for (int v = 0; v < 3; ++v)
        if (outs[v])
            HIPCHK(c, hipMemcpyAsync(outs[v], vecs + (size_t)v * f->npad, sizeof(double) * f->n,
                                     hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (total)
        *total = f->loo_total;
    return BQ_OK;
}

// dL_loo / dtheta in the gradient's parameter order: the Hessian's products stage (fit_prod), then
// one read of its matrices for the row sums and one workgroup for the d + 2 entries.  Both
// workspaces are allocated before anything is launched.
extern "C" int bq_gp_loo_grad(bq_ctx *c, bq_fit *f, double *total, double *grad)
{
    BQCHK(check_fit(c, f));
    if (!grad)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d;
    if (!(f->have & bq_fit::LOO_GRAD)) {
        BQCHK(fit_hess_ws(c, f));
        BQCHK(fit_loo_ws(c, f));
        BQCHK(fit_loo(c, f));
        BQCHK(fit_prod(c, f));
        const double *gd = nullptr;
        BQCHK(launch_loo_grad(c, d, f->gX.d(), f->hB.d(), f->alpha.d(), f->n, f->npad, f->h, f->s,
                              f->g.s2, f->loo.d(), &gd));
        HIPCHK(c, hipMemcpyAsync(f->loo_grad, gd, sizeof(double) * (d + 2), hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        f->have |= bq_fit::LOO_GRAD;
    }
    for (int p = 0; p < d + 2; ++p)
        grad[p] = f->loo_grad[p];
    if (total)
        *total = f->loo_total;
    return BQ_OK;
}

static_assert(BQ_LGO_MAX == 64, "lgo.h's blocks are rows of 64 doubles");

// the groups of one leave-group-out call, checked, as the device reads them
struct LgoGroups {
    std::vector<int> buf; // idx (T) | start (G + 1) | the pivot flag, cleared | bundle (NB + 1)
    long T = 0, G = 0, NB = 0; // NB bundles: consecutive groups of at most BQ_LGO_MAX members together
    int maxb = 0;              // the largest bundle
};

static int lgo_groups(bq_ctx *c, const bq_fit *f, const int64_t *idx, const int64_t *start,
                      int64_t G, LgoGroups &g)
{
    const int n = f->n;
    if (!idx || !start || G < 1 || G > n || start[0] != 0)
        return fail(c, BQ_ERR_BAD_ARG, "lgo: 1 <= G <= n groups, start[0] == 0");
    for (int64_t q = 0; q < G; ++q) {
        const int64_t b = start[q + 1] - start[q];
        if (b < 1 || b > BQ_LGO_MAX)
            return fail(c, BQ_ERR_BAD_ARG, "lgo: group %lld has %lld members, not 1 .. %d",
                        (long long)q, (long long)b, BQ_LGO_MAX);
        if (start[q + 1] > n)
            return fail(c, BQ_ERR_BAD_ARG, "lgo: more members than the fit's %d points", n);
    }
    g.T = (long)start[G];
    g.G = (long)G;
    std::vector<char> seen;
    try {
        seen.assign((size_t)n, 0);
        g.buf.assign((size_t)(g.T + 2 * g.G + 3), 0);
    } catch (const std::bad_alloc &) {
        return fail(c, BQ_ERR_NOMEM, "out of host memory");
    }
    for (long t = 0; t < g.T; ++t) {
        if (idx[t] < 0 || idx[t] >= n)
            return fail(c, BQ_ERR_BAD_ARG, "lgo: index %lld out of range [0, %d)",
                        (long long)idx[t], n);
        if (seen[(size_t)idx[t]])
            return fail(c, BQ_ERR_BAD_ARG, "lgo: index %lld given twice", (long long)idx[t]);
        seen[(size_t)idx[t]] = 1;
        g.buf[(size_t)t] = (int)idx[t];
    }
    for (long q = 0; q <= g.G; ++q)
        g.buf[(size_t)(g.T + q)] = (int)start[q];
    int *bundle = g.buf.data() + g.T + g.G + 2;
    for (long q = 0, first = 0; q <= g.G; ++q)
        if (q == g.G || start[q + 1] - start[first] > BQ_LGO_MAX) { // group q opens the next bundle
            g.maxb = std::max(g.maxb, (int)(start[q] - start[first]));
            bundle[++g.NB] = (int)q;
            first = q;
        }
    return BQ_OK;
}

// The value stage of both entry points, the same launches in both: mu, var, lp and the groups'
// Sigma_B and r_B in the workspace, *total on the host.  Every workspace (with grad: the
// Hessian's too) is there before anything runs.
static int fit_lgo(bq_ctx *c, bq_fit *f, const LgoGroups &g, bool grad, LgoWs &w, double *total)
{
    const int d = f->d, npad = f->npad;
    if (grad)
        BQCHK(fit_hess_ws(c, f));
    BQCHK(fit_grow(c, f->lgo, sizeof(double) * lgo_ws_doubles(npad, d, g.T, g.G, grad),
                   "leave-group-out workspace"));
    BQCHK(fit_alpha(c, f));
    BQCHK(fit_y(c, f));
    w = lgo_views(f->lgo.d(), npad, d, g.T, g.G);
    HIPCHK(c, hipMemcpyAsync(w.idx, g.buf.data(), sizeof(int) * g.buf.size(), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    BQCHK(launch_lgo(c, f->gY.d(), f->alpha.d(), f->y.d(), f->n, npad, d, g.T, g.G, g.NB, g.maxb, w));
    int flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, w.flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(total, w.out, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (flag)
        return fail(c, BQ_ERR_NOT_PD,
                    "lgo: a group's block of Kxx^-1 has a pivot that is not positive and finite");
    return BQ_OK;
}

// Leave-group-out cross-validation (lgo.h has the formulas): the predictive mean and variance of
// every member of every group from the points outside its group, each group's joint log density
// and their sum, from the groups' blocks of Kxx^-1 = Y Y^T and alpha.  Nothing is kept between
// calls but the workspace.
extern "C" int bq_gp_lgo(bq_ctx *c, bq_fit *f, const int64_t *idx, const int64_t *start, int64_t G,
                         double *mean, double *var, double *logpred, double *total)
{
    BQCHK(check_fit(c, f));
    if (!mean && !var && !logpred && !total)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    LgoGroups g;
    BQCHK(lgo_groups(c, f, idx, start, G, g));
    HIPCHK(c, hipSetDevice(c->device));
    LgoWs w;
    double tot = 0.0;
    BQCHK(fit_lgo(c, f, g, false, w, &tot));
    if (mean)
        HIPCHK(c, hipMemcpyAsync(mean, w.mu, sizeof(double) * g.T, hipMemcpyDeviceToHost, c->stream));
    if (var)
        HIPCHK(c, hipMemcpyAsync(var, w.var, sizeof(double) * g.T, hipMemcpyDeviceToHost, c->stream));
    if (logpred)
        HIPCHK(c, hipMemcpyAsync(logpred, w.lp, sizeof(double) * g.G, hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (total)
        *total = tot;
    return BQ_OK;
}

// dL_lgo / dtheta in the gradient's parameter order: the value stage, the Hessian's products stage
// (fit_prod), then the groups' blocks of Q and of the M_k and one workgroup per group for its d + 2
// entries.
extern "C" int bq_gp_lgo_grad(bq_ctx *c, bq_fit *f, const int64_t *idx, const int64_t *start,
                              int64_t G, double *total, double *grad)
{
    BQCHK(check_fit(c, f));
    if (!grad)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    LgoGroups g;
    BQCHK(lgo_groups(c, f, idx, start, G, g));
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d;
    LgoWs w;
    double tot = 0.0;
    BQCHK(fit_lgo(c, f, g, true, w, &tot));
    BQCHK(fit_prod(c, f));
    BQCHK(launch_lgo_grad(c, d, f->gX.d(), f->hB.d(), f->n, f->npad, g.T, g.G, g.NB, g.maxb, f->h, f->s,
                          f->g.s2, w));
    double gd[BQ_MAXD + 2];
    HIPCHK(c, hipMemcpyAsync(gd, w.out + 1, sizeof(double) * (d + 2), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int p = 0; p < d + 2; ++p)
        grad[p] = gd[p];
    if (total)
        *total = tot;
    return BQ_OK;
}

extern "C" int bq_gp_get(bq_ctx *c, bq_fit *f, int which, double *out)
{
    BQCHK(check_fit(c, f));
    if (!out)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    const int n = f->n;
    switch (which) {
    case 0: { // L, strict upper zeroed
        HIPCHK(c, hipMemcpy2DAsync(out, sizeof(double) * n, f->A.p, sizeof(double) * f->ldl,
                                   sizeof(double) * n, n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int j = 1; j < n; ++j)
            for (int i = 0; i < j; ++i)
                out[i + (size_t)j * n] = 0.0;
        return BQ_OK;
    }
    case 1:
        BQCHK(fit_alpha(c, f));
        HIPCHK(c, hipMemcpyAsync(out, f->alpha.p, sizeof(double) * n, hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BQ_OK;
    case 2:
        HIPCHK(c, hipMemcpy2DAsync(out, sizeof(double), f->A.d() + f->L.yrow,
                                   sizeof(double) * f->ldl, sizeof(double), n,
                                   hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BQ_OK;
    case 3: {
        DevBuf K;
        HIPCHK(c, K.alloc(sizeof(double) * (size_t)n * n));
        BQCHK(launch_gram_sym(c, f->d, f->pts.d(), 0, static_cast<GaussParams *>(f->gp.p), 0,
                              K.d(), n, 0, n, 1));
        HIPCHK(c, hipMemcpyAsync(out, K.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BQ_OK;
    }
    default:
        return fail(c, BQ_ERR_BAD_ARG, "unknown item %d", which);
    }
}

namespace bqh {

// whether the cross Gram may read the points out of the mapped staging buffer (bq_gp_predict says
// why there is a limit)
static bool predict_direct_ok(int d, int64_t M, int npad)
{
    return (size_t)d * M * sizeof(double) * (size_t)(npad / 64) <= ((size_t)4 << 20);
}

// The staging of a posterior call (bq_gp_predict, bq_gp_predict_grad, bq_gp_predict_dtheta): M
// points in, results [mean (Mp) | var (Mp) | dmean (nd Mp) | dvar (nd Mp)] out, Mp = M rounded up
// to 64, nd gradient rows per point.  Three routes, chosen once in begin():
//   direct   the kernels read the points out of the mapped pinned staging and write the results
//            into it (the caller asks for it; predict_direct_ok has the limit);
//   flow     one kernel copies the points down, one the results up (launch_flow_in / _out);
//   copies   the same by the copy engine (no kernel copies: BQ_SOLVE_KCOPY=0).
struct PosteriorIO {
    bq_fit *f = nullptr;
    int64_t M = 0;
    int Mp = 0, nd = 0;
    bool direct = false;
    Staging st;                // the points, then the results
    const double *xq = nullptr; // where the kernels read the points (d x M)
    double *res = nullptr;      // where they write the results

    int begin(bq_ctx *c, bq_fit *fit, const double *xo, int64_t M_, int nd_, bool want_direct)
    {
        f = fit, M = M_, nd = nd_;
        Mp = (int)roundup(M, 64);
        const int d = f->d;
        const size_t npts = (size_t)d * M, nres = (2 + 2 * (size_t)nd) * Mp;
        // workspaces live in the fit and only grow: a BQ object predicts thousands of times
        BQCHK(fit_grow(c, f->wx, sizeof(double) * npts, "prediction points"));
        BQCHK(fit_grow(c, f->wout, sizeof(double) * nres, "prediction results"));
        // points up and results down through pinned staging (asynchronous for real)
        if (f->hio_len < npts + nres) {
            if (f->hio)
                (void)hipHostFree(f->hio);
            f->hio = nullptr;
            f->hio_len = 0;
            HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&f->hio),
                                    sizeof(double) * (npts + nres)));
            f->hio_len = npts + nres;
        }
        std::memcpy(f->hio, xo, sizeof(double) * npts);
        BQCHK(stage_view(c, f->hio, st));
        direct = want_direct && st.dev && predict_direct_ok(d, M, f->npad);
        if (direct) {
            xq = st.dev, res = st.dev + npts;
            return BQ_OK;
        }
        xq = f->wx.d(), res = f->wout.d();
        if (st.dev)
            return launch_flow_in(c, st.dev, (int)npts, f->wx.d(), (int)npts, nullptr, 0);
        HIPCHK(c, hipMemcpyAsync(f->wx.p, st.host, sizeof(double) * npts, hipMemcpyHostToDevice,
                                 c->stream));
        return BQ_OK;
    }

    // the first nout doubles of the results back, the stream synchronised, the segments asked for
    // handed out (dmean, dvar: nd x M each)
    int finish(bq_ctx *c, size_t nout, double *mean, double *var, double *dmean, double *dvar)
    {
        const size_t npts = (size_t)f->d * M;
        const double *hres = st.host + npts;
        if (direct)
            ;
        else if (st.dev)
            BQCHK(launch_flow_out(c, res, (int)nout, st.dev + npts));
        else
            HIPCHK(c, hipMemcpyAsync(st.host + npts, res, sizeof(double) * nout,
                                     hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (mean)
            std::memcpy(mean, hres, sizeof(double) * M);
        if (var)
            std::memcpy(var, hres + Mp, sizeof(double) * M);
        if (dmean)
            std::memcpy(dmean, hres + 2 * (size_t)Mp, sizeof(double) * nd * M);
        if (dvar)
            std::memcpy(dvar, hres + (2 + (size_t)nd) * Mp, sizeof(double) * nd * M);
        return BQ_OK;
    }
};

// The sweep of a posterior with its variance: V = K(xo, x) L^-T into f->wV2 (Mp x npad, ld Mp,
// Mp = M rounded up to 64) by a forward sweep with rows = prediction points, f->wV left holding
// the sweep's partial sums; mean (Mp) | var (Mp) at io.res.  With io.direct the points are in the
// mapped staging buffer, which the cross Gram then reads itself and pads by itself.
// (predict_v: everything but the row reductions, which bq_gp_predict_trend runs in its own form)
static int predict_v(bq_ctx *c, bq_fit *f, const PosteriorIO &io);
static int predict_sweep(bq_ctx *c, bq_fit *f, const PosteriorIO &io)
{
    BQCHK(predict_v(c, f, io));
    return launch_rowdot(c, f->wV2.d(), (long)io.Mp, (int)io.M, io.Mp, f->npad, f->wz.d(), f->g.c,
                         io.res, io.res + io.Mp, 1);
}

// z lives in row yrow of the factor with stride ldl: gathered once per (re)fit
int fit_zc(bq_ctx *c, bq_fit *f)
{
    if (!(f->have & bq_fit::ZC)) {
        BQCHK(fit_grow(c, f->wz, sizeof(double) * (size_t)f->npad, "contiguous z"));
        BQCHK(launch_gather_row(c, f->wz.d(), f->A.d() + f->L.yrow, f->ldl, f->npad));
        f->have |= bq_fit::ZC;
    }
    return BQ_OK;
}

static int predict_v(bq_ctx *c, bq_fit *f, const PosteriorIO &io)
{
    const int d = f->d, n = f->n, npad = f->npad, M = (int)io.M, Mp = io.Mp;
    const GaussParams g = f->g;
    WideInv wi;
    BQCHK(fit_wide(c, f, wi));
    DevBuf &V0 = f->wV, &V = f->wV2;
    BQCHK(fit_grow(c, V0, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
    BQCHK(fit_grow(c, V, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
    if (io.direct) {
        BQCHK(launch_gram_cross_pad(c, d, io.xq, M, Mp, f->pts.d(), n, npad, g, V0.d(), Mp));
    } else {
        HIPCHK(c, hipMemsetAsync(V0.p, 0, sizeof(double) * (size_t)Mp * npad, c->stream));
        BQCHK(launch_gram_cross(c, d, io.xq, M, f->pts.d(), n, g, V0.d(), Mp));
    }
    BQCHK(enqueue_forward_rows(c, V0.d(), V.d(), Mp, Mp, f->A.d(), f->ldl, npad, wi));
    return fit_zc(c, f);
}

// beta = V L^-1 out of V (f->wV2) into the buffer the cross Gram came in (f->wV: the forward sweep
// left partial sums there; V is consumed, so the row reductions ran first)
static int predict_beta(bq_ctx *c, bq_fit *f, int Mp)
{
    WideInv wi;
    BQCHK(fit_wide(c, f, wi));
    return enqueue_backward_rows(c, f->wV2.d(), f->wV.d(), Mp, Mp, f->A.d(), f->ldl, f->npad, wi);
}

// Sigma = K(xo, xo) - V V^T, the posterior covariance of the latent function (no s^2), after
// predict_sweep: Mp x Mp, ld Mp, into C; its padding rows and columns are zero.  gd: device room
// for the kernel parameters without s^2.  (bq_gp_predict's cov, bq_gp_sample)
static int posterior_sigma(bq_ctx *c, bq_fit *f, const PosteriorIO &io, double *C, GaussParams *gd)
{
    const int Mp = io.Mp;
    GaussParams g0 = f->g;
    g0.s2 = 0.0;
    HIPCHK(c, hipMemsetAsync(C, 0, sizeof(double) * (size_t)Mp * Mp, c->stream));
    HIPCHK(c, hipMemcpyAsync(gd, &g0, sizeof g0, hipMemcpyHostToDevice, c->stream));
    BQCHK(launch_gram_sym(c, f->d, io.xq, 0, gd, 0, C, Mp, 0, (int)io.M, 1));
    GemmJob vvt;
    vvt.C = C, vvt.ldc = Mp;
    vvt.P = f->wV2.d(), vvt.ldp = Mp;
    vvt.Q = f->wV2.d(), vvt.qsj = 1, vvt.qsk = Mp;
    vvt.m = Mp, vvt.n = Mp, vvt.k = f->npad;
    return launch_gemm(c, BQ_K_GEMM, vvt);
}

// what the three posterior entry points check alike; *none: there is nothing to do
static int predict_args(bq_ctx *c, bq_fit *f, const double *xo, int64_t M, bool any_out, bool *none)
{
    BQCHK(check_fit(c, f));
    if (M < 0 || (M && !xo) || !any_out)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    *none = M == 0;
    if (M)
        HIPCHK(c, hipSetDevice(c->device));
    return BQ_OK;
}

} // namespace bqh

extern "C" int bq_gp_predict(bq_ctx *c, bq_fit *f, const double *xo, int64_t M, double *mean,
                             double *var, double *cov)
{
    bool none;
    BQCHK(predict_args(c, f, xo, M, true, &none));
    if (none)
        return BQ_OK;
    const int d = f->d, n = f->n;
    if (!var && !cov)
        BQCHK(fit_alpha(c, f));
    // mean + variance without the covariance (BQ.l_var, _set_gp_log_l_params: bq.py:227-228,
    // 942-943) is six launches: the cross Gram reads the points out of the mapped staging buffer
    // and writes its own zero padding, the row reductions write the results into it (round 5:
    // flow_in, the memset and flow_out gone, 59 -> 48 us of kernels at N = 1024, M = 256)
    // (every workgroup column of the cross Gram re-reads the points over PCIe: npad / 64 uncached
    // passes over d M doubles.  Measured a win at N = 1024, M = 256 / 1000; above a few MB of such
    // reads the points go down once through flow_in instead -- ADVICE r05)
    PosteriorIO io;
    BQCHK(io.begin(c, f, xo, M, 0, var && !cov));
    const int Mp = io.Mp;
    const GaussParams g = f->g;
    if (!var && !cov) {
        // mean only: fused cross-Gram x alpha
        BQCHK(launch_predict_mean(c, d, io.xq, (int)M, f->pts.d(), n, f->alpha.d(), g, io.res));
    } else {
        BQCHK(predict_sweep(c, f, io));
        if (cov) {
            // cov = K(xo,xo) - V V^T  (Mp x Mp on device, M x M out)
            DevBuf Cd, gd;
            HIPCHK(c, Cd.alloc(sizeof(double) * (size_t)Mp * Mp));
            HIPCHK(c, gd.alloc(sizeof(GaussParams)));
            BQCHK(posterior_sigma(c, f, io, Cd.d(), static_cast<GaussParams *>(gd.p)));
            HIPCHK(c, hipMemcpy2DAsync(cov, sizeof(double) * M, Cd.p, sizeof(double) * Mp,
                                       sizeof(double) * M, M, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream)); // Cd goes out of scope
        }
    }
    return io.finish(c, 2 * (size_t)Mp, mean, var, nullptr, nullptr); // [mean | var], one copy
}

// The posterior and its gradients with respect to the query points (pgrad.h has the formulas).
// Mean route (no var, no dvar): alpha, then one fused launch, no sweep and no M x n matrix.  Full
// route: bq_gp_predict's own staging, cross Gram, forward sweep and row reductions (predict_sweep:
// mean and var are bq_gp_predict's bits), then -- for dvar -- the backward row sweep
// beta = V L^-1 (predict_beta), and one launch over beta, alpha and the points.
// Results: [mean (Mp) | var (Mp) | dmean (d Mp) | dvar (d Mp)].
extern "C" int bq_gp_predict_grad(bq_ctx *c, bq_fit *f, const double *xo, int64_t M, double *mean,
                                  double *var, double *dmean, double *dvar)
{
    bool none;
    BQCHK(predict_args(c, f, xo, M, mean || var || dmean || dvar, &none));
    if (none)
        return BQ_OK;
    const int d = f->d, n = f->n;
    const bool full = var || dvar;
    // (alpha first: the call that builds it synchronises, which would split the chain below)
    if (!full || dmean)
        BQCHK(fit_alpha(c, f));
    // the full route stages its points as bq_gp_predict does for mean + variance
    PosteriorIO io;
    BQCHK(io.begin(c, f, xo, M, d, full));
    const int Mp = io.Mp;
    double *odm = io.res + 2 * (size_t)Mp, *odv = odm + (size_t)d * Mp;
    size_t nout = 2 * (size_t)Mp; // how much of the results goes back
    if (!full) {
        BQCHK(launch_predict_mean_grad(c, d, io.xq, (int)M, f->pts.d(), n, f->alpha.d(), f->g,
                                       io.res, odm));
        nout += (size_t)d * Mp;
    } else {
        BQCHK(predict_sweep(c, f, io));
        if (dvar)
            BQCHK(predict_beta(c, f, Mp));
        if (dmean || dvar) {
            BQCHK(launch_predict_grad(c, d, dvar ? f->wV.d() : nullptr, (long)Mp, (int)M, Mp, io.xq,
                                      f->pts.d(), n, dmean ? f->alpha.d() : nullptr, f->g,
                                      dmean ? odm : nullptr, dvar ? odv : nullptr));
            nout += 2 * (size_t)d * Mp;
        }
    }
    return io.finish(c, nout, mean, var, dmean, dvar);
}

// The posterior and its derivatives in the hyper-parameters theta = [h, w_1 .. w_d, s] (ptheta.h
// has the formulas).  Mean route (no var, no dvar): alpha and the fit's solved vectors (fit_dkz),
// then one fused launch, no sweep and no M x n matrix.  Full route: both of those first (they
// synchronise), bq_gp_predict's own staging, cross Gram, forward sweep and row reductions
// (predict_sweep: mean and var are bq_gp_predict's bits), then -- for dvar -- the backward row
// sweep beta = V L^-1 (predict_beta) and one MFMA launch per length scale for
// q_jk = beta_j^T D_k beta_j, and one launch over beta, the solved vectors and the points.
// Results: [mean (Mp) | var (Mp) | dmean ((d + 2) Mp) | dvar ((d + 2) Mp)].
extern "C" int bq_gp_predict_dtheta(bq_ctx *c, bq_fit *f, const double *xo, int64_t M,
                                    double *mean, double *var, double *dmean, double *dvar)
{
    bool none;
    BQCHK(predict_args(c, f, xo, M, mean || var || dmean || dvar, &none));
    if (none)
        return BQ_OK;
    const int d = f->d, np = d + 2;
    const bool full = var || dvar;
    // (the fit's own vectors first: building them synchronises, which would split the chain below)
    if (!full || dmean) {
        BQCHK(fit_alpha(c, f));
        BQCHK(fit_dkz(c, f));
    }
    if (dvar)
        BQCHK(fit_grow(c, f->wq,
                       sizeof(double) * ptheta_part_doubles(d, (int)roundup(M, 64), f->npad),
                       "hyper-parameter derivative partial sums"));
    // the full route stages its points as bq_gp_predict does for mean + variance
    PosteriorIO io;
    BQCHK(io.begin(c, f, xo, M, np, full));
    const int Mp = io.Mp;
    double *odm = io.res + 2 * (size_t)Mp, *odv = odm + (size_t)np * Mp;
    size_t nout = 2 * (size_t)Mp; // how much of the results goes back
    const HessJob hj = fit_hess_job(f);
    if (!full) {
        BQCHK(launch_predict_mean_theta(c, d, io.xq, (int)M, hj, f->dkz.d(), f->h, f->s, io.res,
                                        odm));
        nout += (size_t)np * Mp;
    } else {
        BQCHK(predict_sweep(c, f, io));
        if (dvar) {
            BQCHK(predict_beta(c, f, Mp));
            BQCHK(launch_ptheta_quad(c, d, f->wV.d(), (long)Mp, Mp, hj, f->wq.d()));
        }
        if (dmean || dvar) {
            BQCHK(launch_predict_theta(c, d, dvar ? f->wV.d() : nullptr, (long)Mp, (int)M, Mp, io.xq,
                                       hj, dmean ? f->dkz.d() : nullptr, io.res + Mp,
                                       dvar ? f->wq.d() : nullptr, f->h, f->s,
                                       dmean ? odm : nullptr, dvar ? odv : nullptr));
            nout += 2 * (size_t)np * Mp;
        }
    }
    return io.finish(c, nout, mean, var, dmean, dvar);
}

// ===========================================================================
// The polynomial trend of a fit, its coefficients marginalised (include/bqhip.h has the contract;
// trend.h the kernels)
// ===========================================================================
namespace bqh {

// the basis of a trend call, checked against the fit: the key of the state (entries from d on are
// fixed, so that two keys compare byte by byte)
static int trend_basis(bq_ctx *c, const bq_fit *f, int degree, const double *center,
                       const double *scale, TrendBasis &tb)
{
    if (degree < 0 || degree > 2)
        return fail(c, BQ_ERR_BAD_ARG, "trend: degree %d, not 0 .. 2", degree);
    if (!center || !scale)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    tb = TrendBasis{};
    tb.degree = degree;
    tb.p = trend_p(degree, f->d);
    for (int k = 0; k < BQ_MAXD; ++k) {
        tb.c[k] = k < f->d ? center[k] : 0.0;
        tb.rho[k] = k < f->d ? scale[k] : 1.0;
        if (!std::isfinite(tb.c[k]))
            return fail(c, BQ_ERR_BAD_ARG, "trend: the centre must be finite");
        if (!(tb.rho[k] > 0.0) || !std::isfinite(tb.rho[k]))
            return fail(c, BQ_ERR_BAD_ARG, "trend: the scale must be positive and finite");
    }
    if (f->n < tb.p)
        return fail(c, BQ_ERR_BAD_ARG, "trend: %d observations for %d basis functions", f->n, tb.p);
    return BQ_OK;
}

static bool trend_current(const bq_fit *f, const TrendBasis &tb)
{
    return (f->have & bq_fit::TREND) && std::memcmp(&f->tr_key, &tb, sizeof tb) == 0;
}

// every buffer the producer touches, there before its first launch
static int trend_alloc(bq_ctx *c, bq_fit *f)
{
    BQCHK(fit_grow(c, f->wide, sizeof(double) * wide_alloc_doubles(f->npad), "wide block inverses"));
    BQCHK(fit_vec(c, f));
    BQCHK(fit_grow(c, f->wz, sizeof(double) * (size_t)f->npad, "contiguous z"));
    return fit_grow(c, f->trend, sizeof(double) * trend_plan(f->npad).total, "trend state");
}

// The producer of TREND, first half: its launches, nothing read back.  H by the basis kernel, G =
// L^-1 H by the forward row sweep with 64 rows (fit_dkz's form), A and b in slices and one fold,
// the one-workgroup solve, which leaves z - G beta in the single-vector workspace, and the
// backward single-vector sweep from there into the state's own alpha_t.  The bit is dropped first:
// the state belongs to no key until fit_trend has seen the status.
static int trend_enqueue(bq_ctx *c, bq_fit *f, const TrendBasis &tb)
{
    const int npad = f->npad;
    const TrendPlan pl = trend_plan(npad);
    double *ws = f->trend.d();
    f->drop(bq_fit::TREND);
    WideInv w;
    BQCHK(fit_wide(c, f, w));
    BQCHK(fit_zc(c, f));
    BQCHK(launch_trend_basis(c, f->d, f->pts.d(), f->n, npad, tb, ws + pl.o_H, 1, BQ_TREND_ROWS));
    BQCHK(enqueue_forward_rows(c, ws + pl.o_H, ws + pl.o_G, BQ_TREND_ROWS, BQ_TREND_ROWS, f->A.d(),
                               f->ldl, npad, w));
    BQCHK(launch_trend_sums(c, ws + pl.o_G, f->wz.d(), npad, tb.p, ws + pl.o_part, ws + pl.o_sums));
    BQCHK(launch_trend_solve(c, ws + pl.o_sums, tb.p, ws + pl.o_G, f->wz.d(), npad, ws + pl.o_tr,
                             f->vec.d()));
    return enqueue_backward_vec(c, f->vec.d(), ws + pl.o_alpha, f->A.d(), f->ldl, npad, w,
                                f->vec.d() + 2 * (size_t)npad);
}

// ... second half, once the stream is synchronised and the solve's status is on the host: the
// state is the key's, or nobody's
static int fit_trend(bq_ctx *c, bq_fit *f, const TrendBasis &tb, double status)
{
    if (status != 0.0) {
        f->drop(bq_fit::TREND);
        return fail(c, BQ_ERR_NOT_PD,
                    "trend: H^T Kxx^-1 H has a pivot that is not positive and finite");
    }
    f->tr_key = tb;
    f->have |= bq_fit::TREND;
    return BQ_OK;
}

} // namespace bqh

extern "C" int bq_gp_trend(bq_ctx *c, bq_fit *f, int degree, const double *center,
                           const double *scale, double *beta, double *cov_beta, double *logml_t,
                           double *alpha_t)
{
    BQCHK(check_fit(c, f));
    TrendBasis tb;
    BQCHK(trend_basis(c, f, degree, center, scale, tb));
    if (!beta && !cov_beta && !logml_t && !alpha_t)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    BQCHK(trend_alloc(c, f));
    double *hs, *ds;
    BQCHK(ctx_stage(c, BQ_TREND_HEAD, &hs, &ds));
    const int p = tb.p, n = f->n;
    const bool fresh = !trend_current(f, tb);
    const TrendPlan pl = trend_plan(f->npad);
    const double *ws = f->trend.d();
    // one read-back: the head of the state and alpha_t into pinned staging
    BQCHK(with_flow_fallback(c, [&]() -> int {
        if (fresh)
            BQCHK(trend_enqueue(c, f, tb));
        HIPCHK(c, hipMemcpyAsync(hs, ws + pl.o_tr, sizeof(double) * BQ_TREND_HEAD,
                                 hipMemcpyDeviceToHost, c->stream));
        if (alpha_t)
            HIPCHK(c, hipMemcpyAsync(f->hvec, ws + pl.o_alpha, sizeof(double) * n,
                                     hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BQ_OK;
    }));
    BQCHK(fit_trend(c, f, tb, hs[BQ_TREND_STATUS]));
    if (beta)
        std::memcpy(beta, hs + BQ_TREND_BETA, sizeof(double) * p);
    if (cov_beta)
        std::memcpy(cov_beta, hs + BQ_TREND_AINV, sizeof(double) * p * p);
    if (logml_t)
        *logml_t = -0.5 * (f->qf - hs[BQ_TREND_BTB]) - 0.5 * f->logdet - 0.5 * hs[BQ_TREND_LOGDET] -
                   0.5 * (double)(n - p) * 1.8378770664093453; // log 2 pi
    if (alpha_t)
        std::memcpy(alpha_t, f->hvec, sizeof(double) * n);
    return BQ_OK;
}

// The trend posterior at M points.  Mean route (no var): the state, then one fused launch over
// alpha_t, no sweep and no M x n matrix.  Full route: bq_gp_predict's staging, cross Gram and
// forward sweep (predict_v), the basis rows of the points, then the row reductions with the p
// sums v_j.G_k in the same pass (trend_route: p <= 8) or bq_gp_predict's own reductions and one
// product R = Phi - V G^T, and one finishing launch.  Where the state is not there for this key its
// producer is enqueued in front: either way one read-back, which carries the solve's status.
extern "C" int bq_gp_predict_trend(bq_ctx *c, bq_fit *f, int degree, const double *center,
                                   const double *scale, const double *xo, int64_t M, double *mean,
                                   double *var)
{
    BQCHK(check_fit(c, f));
    TrendBasis tb;
    BQCHK(trend_basis(c, f, degree, center, scale, tb));
    if (M < 0 || (M && !xo) || (!mean && !var))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (M == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d, n = f->n, npad = f->npad, p = tb.p, Mp = (int)roundup(M, 64);
    const bool full = var != nullptr;
    const TrendRoute route = trend_route(p, full);
    BQCHK(trend_alloc(c, f));
    if (full) {
        BQCHK(fit_grow(c, f->wV, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
        BQCHK(fit_grow(c, f->wV2, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
        BQCHK(fit_grow(c, f->wphi, sizeof(double) * (size_t)Mp * BQ_TREND_ROWS,
                       "basis rows of the prediction points"));
    }
    const bool fresh = !trend_current(f, tb);
    const TrendPlan pl = trend_plan(npad);
    const double *ws = f->trend.d(), *G = ws + pl.o_G, *tr = ws + pl.o_tr;
    PosteriorIO io;
    GemmRoute ran{};
    BQCHK(with_flow_fallback(c, [&]() -> int {
        if (fresh)
            BQCHK(trend_enqueue(c, f, tb));
        BQCHK(io.begin(c, f, xo, M, 1, full)); // (nd = 1: room for the status behind mean | var)
        double *status = io.res + 2 * (size_t)Mp;
        if (!full) {
            BQCHK(launch_trend_mean(c, d, io.xq, (int)M, f->pts.d(), n, ws + pl.o_alpha, f->g, tb, tr,
                                    io.res, status));
        } else {
            BQCHK(predict_v(c, f, io));
            double *R = f->wphi.d();
            BQCHK(launch_trend_basis(c, d, io.xq, (int)M, Mp, tb, R, Mp, 1));
            if (route == TrendRoute::OnePass) {
                BQCHK(launch_rowdot_trend(c, f->wV2.d(), (long)Mp, (int)M, Mp, npad, f->wz.d(),
                                          f->g.c, G, p, io.res, io.res + Mp, R));
            } else {
                BQCHK(launch_rowdot(c, f->wV2.d(), (long)Mp, (int)M, Mp, npad, f->wz.d(), f->g.c,
                                    io.res, io.res + Mp, 1));
                GemmJob vg;
                vg.C = R, vg.ldc = Mp;
                vg.P = f->wV2.d(), vg.ldp = Mp;
                vg.Q = G, vg.qsj = 1, vg.qsk = BQ_TREND_ROWS;
                vg.m = Mp, vg.n = BQ_TREND_ROWS, vg.k = npad;
                BQCHK(launch_gemm(c, BQ_K_GEMM, vg, &ran));
            }
            BQCHK(launch_trend_finish(c, R, (long)Mp, (int)M, p, tr, io.res, io.res + Mp, status));
        }
        return io.finish(c, 2 * (size_t)Mp + 1, nullptr, nullptr, nullptr, nullptr);
    }));
    const double *hres = io.st.host + (size_t)d * M;
    BQCHK(fit_trend(c, f, tb, hres[2 * (size_t)Mp]));
    f->tr_route = (int)route;
    f->tr_gemm = route == TrendRoute::Gemm ? (int)ran.kernel : -1;
    if (mean)
        std::memcpy(mean, hres, sizeof(double) * M);
    if (var)
        std::memcpy(var, hres + Mp, sizeof(double) * M);
    return BQ_OK;
}

extern "C" int bq_gp_trend_last_route(bq_ctx *c, bq_fit *f, int *route, int *gemm_kernel)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!f || !route)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    *route = f->tr_route;
    if (gemm_kernel)
        *gemm_kernel = f->tr_gemm;
    return BQ_OK;
}

// S joint draws of the latent posterior at M points (include/bqhip.h has the contract; sample.h the
// kernels).  bq_gp_predict's staging, sweep and Sigma (posterior_sigma), formed once; then per
// ladder entry a copy of Sigma (none when the ladder has one entry: Sigma itself is factored), the
// jitter on its first M diagonal entries, potrf_one and one read of info; then the normals
// (uploaded, or normal_fill_kernel), tri_sample_kernel and the downloads.  The factorisation writes
// the lower triangle alone: above the diagonal the factored matrix still holds Sigma, which the
// product masks and the host zeroes in chol.  Every device buffer is there before the first
// launch, and nothing reaches the caller's memory unless a ladder entry has factored.
extern "C" int bq_gp_sample(bq_ctx *c, bq_fit *f, const double *xo, int64_t M, int64_t S,
                            const double *z, uint64_t seed, const double *ladder, int64_t nl,
                            double *out, double *mean, double *chol, double *jitter)
{
    static const double default_ladder[5] = {0.0, 1e-12, 1e-10, 1e-8, 1e-6};
    BQCHK(check_fit(c, f));
    if (M < 0 || S < 1 || M > BQ_SAMPLE_MAX_M || S > BQ_SAMPLE_MAX_S || !out || (M && !xo))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (!ladder) {
        ladder = default_ladder;
        nl = 5;
    }
    if (nl < 1)
        return fail(c, BQ_ERR_BAD_ARG, "sample: a ladder holds at least one entry");
    for (int64_t t = 0; t < nl; ++t)
        if (!std::isfinite(ladder[t]))
            return fail(c, BQ_ERR_BAD_ARG, "sample: ladder entries must be finite");
    if (M == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d, npad = f->npad, m = (int)M, ns = (int)S, Mp = (int)roundup(M, 64);
    const size_t mm = (size_t)Mp * Mp, ms = (size_t)Mp * ns;

    // ---- every device buffer: the sample's own, the prediction's, the factorisation's
    auto granule = [](size_t doubles) { return (doubles + 31) & ~(size_t)31; };
    const size_t ogp = 0, oinfo = granule((sizeof(GaussParams) + 7) / 8), osig = oinfo + 32,
                 owork = osig + mm, oz = owork + (nl > 1 ? mm : 0), oout = oz + granule(ms);
    BQCHK(fit_grow(c, f->smp, sizeof(double) * (oout + ms), "posterior sample workspace"));
    BQCHK(fit_grow(c, f->wide, sizeof(double) * wide_alloc_doubles(npad), "wide block inverses"));
    BQCHK(fit_grow(c, f->wV, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
    BQCHK(fit_grow(c, f->wV2, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
    BQCHK(fit_grow(c, f->wz, sizeof(double) * (size_t)npad, "contiguous z"));
    BQCHK(fit_grow(c, f->wx, sizeof(double) * (size_t)d * M, "prediction points"));
    BQCHK(fit_grow(c, f->wout, sizeof(double) * 2 * (size_t)Mp, "prediction results"));
    BQCHK(grow_panel_ws(c, Mp));
    if (!c->dinv64.p)
        HIPCHK(c, c->dinv64.alloc(BQ_DINV_STRIDE * sizeof(double)));
    double *base = f->smp.d(), *Sig = base + osig, *W = nl > 1 ? base + owork : Sig, *Z = base + oz,
           *O = base + oout;
    int *info = reinterpret_cast<int *>(base + oinfo);

    // ---- mean | var at io.res, V in f->wV2, Sigma with the identity on its padding diagonal
    PosteriorIO io;
    BQCHK(io.begin(c, f, xo, M, 0, false));
    BQCHK(predict_sweep(c, f, io));
    BQCHK(posterior_sigma(c, f, io, Sig, reinterpret_cast<GaussParams *>(base + ogp)));
    if (Mp > m)
        BQCHK(launch_sample_diag(c, Sig, Mp, m, Mp, 0.0));

    // ---- the first ladder entry whose matrix factors
    double jit = 0.0;
    int64_t t = 0;
    for (; t < nl; ++t) {
        jit = f->g.c * ladder[t];
        if (nl > 1)
            HIPCHK(c, hipMemcpyAsync(W, Sig, sizeof(double) * mm, hipMemcpyDeviceToDevice,
                                     c->stream));
        if (jit != 0.0)
            BQCHK(launch_sample_diag(c, W, Mp, m, Mp, jit));
        HIPCHK(c, hipMemsetAsync(info, 0, sizeof(int), c->stream));
        BQCHK(potrf_one(c, W, Mp, Mp, c->dinv64.d(), info));
        int hinfo = 0;
        HIPCHK(c, hipMemcpyAsync(&hinfo, info, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (hinfo == 0)
            break;
    }
    if (t == nl)
        return fail(c, BQ_ERR_NOT_PD,
                    "sample: the posterior covariance did not factor with any of the %lld jitters",
                    (long long)nl);

    // ---- the normals, the product, the downloads
    if (z) {
        HIPCHK(c, hipMemsetAsync(Z, 0, sizeof(double) * ms, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(Z, sizeof(double) * Mp, z, sizeof(double) * M,
                                   sizeof(double) * M, S, hipMemcpyHostToDevice, c->stream));
    } else {
        BQCHK(launch_normal_fill(c, Z, Mp, m, Mp, ns, seed));
    }
    BQCHK(launch_tri_sample(c, W, Mp, Z, Mp, io.res, O, Mp, m, Mp, ns));
    HIPCHK(c, hipMemcpy2DAsync(out, sizeof(double) * M, O, sizeof(double) * Mp, sizeof(double) * M,
                               S, hipMemcpyDeviceToHost, c->stream));
    if (chol)
        HIPCHK(c, hipMemcpy2DAsync(chol, sizeof(double) * M, W, sizeof(double) * Mp,
                                   sizeof(double) * M, M, hipMemcpyDeviceToHost, c->stream));
    BQCHK(io.finish(c, 2 * (size_t)Mp, mean, nullptr, nullptr, nullptr));
    if (chol)
        for (int64_t j = 1; j < M; ++j)
            for (int64_t i = 0; i < j; ++i)
                chol[i + j * M] = 0.0;
    if (jitter)
        *jitter = jit;
    return BQ_OK;
}

// The pivoted partial Cholesky of the posterior covariance at M points (include/bqhip.h has the
// contract; pivchol.h the kernels).  bq_gp_predict's staging and sweep with q more columns behind
// V in f->wV2 -- W = [V | C] is one matrix, ld Mp -- then the start and the q steps, enqueued one
// after the other with nothing read back in between: the pivot and the done flag stay on the
// device, and after the flag a step's kernels return at once.  One download of the workspace's
// head (state | gain | piv | d) into pinned staging and one synchronise; then the rank columns of
// C.  Every device buffer is there before the first launch.
extern "C" int bq_gp_pivchol(bq_ctx *c, bq_fit *f, const double *xo, int64_t M, int64_t q,
                             double nugget, double tol, int64_t *piv, double *C, double *resid,
                             double *gain, int64_t *rank)
{
    BQCHK(check_fit(c, f));
    if (M < 0 || q < 1 || (M && q > M) || M > BQ_PIVCHOL_MAX_M || q > BQ_PIVCHOL_MAX_Q ||
        !(nugget >= 0.0) || !(tol >= 0.0) || !std::isfinite(nugget) || !std::isfinite(tol) ||
        !piv || !gain || !rank || (M && !xo))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (M == 0) {
        for (int64_t j = 0; j < q; ++j)
            piv[j] = -1, gain[j] = 0.0;
        *rank = 0;
        return BQ_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d, npad = f->npad, m = (int)M, nq = (int)q, Mp = (int)roundup(M, 64);
    const PivcholPlan pl = pivchol_plan(Mp, npad, nq);

    // ---- every device buffer: the factorisation's own, the prediction's with q more columns
    BQCHK(fit_grow(c, f->pvc, sizeof(double) * pl.total, "pivoted Cholesky workspace"));
    BQCHK(fit_grow(c, f->wide, sizeof(double) * wide_alloc_doubles(npad), "wide block inverses"));
    BQCHK(fit_grow(c, f->wV, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
    BQCHK(fit_grow(c, f->wV2, sizeof(double) * (size_t)Mp * ((size_t)npad + nq),
                   "prediction sweep workspace and the factor's columns"));
    BQCHK(fit_grow(c, f->wz, sizeof(double) * (size_t)npad, "contiguous z"));
    double *hs, *ds;
    BQCHK(ctx_stage(c, pl.head, &hs, &ds));
    double *ws = f->pvc.d(), *W = f->wV2.d();

    // ---- mean | var at io.res, V in the first npad columns of W; the factor's columns zero
    PosteriorIO io;
    BQCHK(io.begin(c, f, xo, M, 0, false));
    BQCHK(predict_sweep(c, f, io));
    HIPCHK(c, hipMemsetAsync(W + (size_t)Mp * npad, 0, sizeof(double) * (size_t)Mp * nq, c->stream));

    // ---- the steps
    const double thr = tol * f->g.c;
    BQCHK(launch_pivchol_init(c, pl, ws, io.res + Mp, m, Mp, nq, thr));
    for (int j = 0; j < nq; ++j)
        BQCHK(launch_pivchol_step(c, pl, ws, W, d, io.xq, f->g, m, Mp, npad, nq, j, nugget, thr));

    // ---- the download
    HIPCHK(c, hipMemcpyAsync(hs, ws, sizeof(double) * pl.head, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int r = reinterpret_cast<const PivcholState *>(hs)->rank;
    if (r < 0 || r > nq)
        return fail(c, BQ_ERR_HIP, "pivchol: the device left rank %d of %d steps", r, nq);
    if (C) {
        if (r > 0)
            HIPCHK(c, hipMemcpy2D(C, sizeof(double) * M, W + (size_t)Mp * npad, sizeof(double) * Mp,
                                  sizeof(double) * M, r, hipMemcpyDeviceToHost));
        std::memset(C + (size_t)M * r, 0, sizeof(double) * (size_t)M * (nq - r));
    }
    std::memcpy(gain, hs + pl.o_gain, sizeof(double) * nq);
    std::memcpy(piv, hs + pl.o_piv, sizeof(int64_t) * nq);
    if (resid)
        std::memcpy(resid, hs + pl.o_d, sizeof(double) * M);
    *rank = r;
    return BQ_OK;
}

// The greedy design that minimises the integrated posterior variance (include/bqhip.h has the
// contract; ivr.h the kernels).  One staging and one sweep over the joint point set [reference
// points, padded to a multiple of 64 by repeating the last one with weight 0 | candidates] -- so
// the candidate rows of V start on a 64-row boundary; xr == NULL: the candidates alone -- with q
// more columns behind V in f->wV2 for the candidates' c.  T = K(xc, xr) - V_c V_r^T by the cross
// Gram and one product (gemm_route picks its kernel), dc and dr the sweep's variances; then the q
// steps, enqueued one after the other with nothing read back in between.  One download of the
// workspace's head into pinned staging and one synchronise.  Every device buffer is there before
// the first launch.
extern "C" int bq_gp_ivr(bq_ctx *c, bq_fit *f, const double *xr, int64_t R, const double *rho,
                         const double *xc, int64_t A, int64_t q, double nugget, double tol,
                         int64_t *piv, double *gain, double *ivar0, double *resid_r,
                         double *resid_c, double *score0, int64_t *rank)
{
    BQCHK(check_fit(c, f));
    const bool self = R == 0 && !xr;
    if (A < 0 || R < 0 || A > BQ_PIVCHOL_MAX_M || R > BQ_PIVCHOL_MAX_M ||
        R + A > BQ_PIVCHOL_MAX_M || q < 1 || (A && q > A) || q > BQ_PIVCHOL_MAX_Q ||
        !(nugget >= 0.0) || !(tol >= 0.0) || !std::isfinite(nugget) || !std::isfinite(tol) ||
        !piv || !gain || !ivar0 || !rank || (A && (!xc || !rho)) || ((R > 0) != (xr != nullptr)))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    const int64_t Ap64 = roundup(A, 64), Rp64 = self ? Ap64 : roundup(R, 64);
    if (Ap64 * Rp64 > BQ_IVR_MAX_CELLS)
        return fail(c, BQ_ERR_BAD_ARG, "ivr: %lld x %lld entries of T, at most %lld",
                    (long long)Ap64, (long long)Rp64, (long long)BQ_IVR_MAX_CELLS);
    const int64_t nw = self ? A : R;
    double wsum = 0.0;
    for (int64_t j = 0; A && j < nw; ++j) {
        if (!(rho[j] >= 0.0) || !std::isfinite(rho[j]))
            return fail(c, BQ_ERR_BAD_ARG, "ivr: weight %lld is negative or not finite",
                        (long long)j);
        wsum += rho[j];
    }
    if (A == 0) {
        for (int64_t j = 0; j < q; ++j)
            piv[j] = -1, gain[j] = 0.0;
        *ivar0 = 0.0;
        *rank = 0;
        return BQ_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d, npad = f->npad, nq = (int)q;
    const IvrPlan pl = ivr_plan((int)A, (int)R, self, npad, nq);
    const int Ap = pl.Ap, Rp = pl.Rp, Mp = pl.Mp;
    const int64_t M = (int64_t)pl.cand0 + A; // the joint set's points

    // ---- the joint point set on the host
    std::vector<double> joint;
    if (!self) {
        try {
            joint.resize((size_t)d * M);
        } catch (const std::bad_alloc &) {
            return fail(c, BQ_ERR_NOMEM, "ivr: the joint point set (%zu bytes)",
                        sizeof(double) * (size_t)d * M);
        }
        std::memcpy(joint.data(), xr, sizeof(double) * (size_t)d * R);
        for (int64_t j = R; j < Rp; ++j)
            std::memcpy(joint.data() + (size_t)d * j, xr + (size_t)d * (R - 1), sizeof(double) * d);
        std::memcpy(joint.data() + (size_t)d * Rp, xc, sizeof(double) * (size_t)d * A);
    }

    // ---- every device buffer: the steps' own, T, the prediction's with q more columns
    BQCHK(fit_grow(c, f->ivr, sizeof(double) * pl.total, "integrated variance workspace"));
    BQCHK(fit_grow(c, f->ivrT, sizeof(double) * (size_t)Ap * Rp,
                   "candidate-reference covariance"));
    BQCHK(fit_grow(c, f->wide, sizeof(double) * wide_alloc_doubles(npad), "wide block inverses"));
    BQCHK(fit_grow(c, f->wV, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
    BQCHK(fit_grow(c, f->wV2, sizeof(double) * (size_t)Mp * ((size_t)npad + nq),
                   "prediction sweep workspace and the candidates' columns"));
    BQCHK(fit_grow(c, f->wz, sizeof(double) * (size_t)npad, "contiguous z"));
    double *hs, *ds;
    BQCHK(ctx_stage(c, pl.head + (size_t)Rp, &hs, &ds));
    double *ws = f->ivr.d(), *W = f->wV2.d(), *T = f->ivrT.d();

    // ---- the weights, 0 on the padding
    double *hrho = hs + pl.head;
    std::memcpy(hrho, rho, sizeof(double) * nw);
    std::fill(hrho + nw, hrho + Rp, 0.0);

    // ---- mean | var at io.res, V in the first npad columns of W
    PosteriorIO io;
    BQCHK(io.begin(c, f, self ? xc : joint.data(), M, 0, false));
    BQCHK(predict_sweep(c, f, io));
    const double *xcd = io.xq + (size_t)d * pl.cand0;
    HIPCHK(c, hipMemcpyAsync(ws + pl.o_rho, hrho, sizeof(double) * Rp, hipMemcpyHostToDevice,
                             c->stream));

    // ---- T = K(xc, xr) - V_c V_r^T; its padding rows stay zero
    HIPCHK(c, hipMemsetAsync(T, 0, sizeof(double) * (size_t)Ap * Rp, c->stream));
    BQCHK(launch_gram_cross(c, d, xcd, (int)A, io.xq, self ? (int)A : Rp, f->g, T, Ap));
    GemmJob vvt;
    vvt.C = T, vvt.ldc = Ap;
    vvt.P = W + pl.cand0, vvt.ldp = Mp;
    vvt.Q = W, vvt.qsj = 1, vvt.qsk = Mp;
    vvt.m = Ap, vvt.n = Rp, vvt.k = npad;
    BQCHK(launch_gemm(c, BQ_K_GEMM, vvt));

    // ---- the steps
    const double thr = tol * f->g.c * wsum;
    BQCHK(launch_ivr_init(c, pl, ws, io.res + Mp));
    for (int t = 0; t < nq; ++t)
        BQCHK(launch_ivr_step(c, pl, ws, T, W, d, xcd, f->g, t, nugget, thr));

    // ---- the download
    HIPCHK(c, hipMemcpyAsync(hs, ws, sizeof(double) * pl.head, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int r = reinterpret_cast<const PivcholState *>(hs)->rank;
    if (r < 0 || r > nq)
        return fail(c, BQ_ERR_HIP, "ivr: the device left rank %d of %d steps", r, nq);
    std::memcpy(gain, hs + pl.o_gain, sizeof(double) * nq);
    std::memcpy(piv, hs + pl.o_piv, sizeof(int64_t) * nq);
    *ivar0 = hs[pl.o_ivar];
    if (resid_r)
        std::memcpy(resid_r, hs + pl.o_dr, sizeof(double) * nw);
    if (resid_c)
        std::memcpy(resid_c, hs + pl.o_dc, sizeof(double) * A);
    if (score0)
        std::memcpy(score0, hs + pl.o_score0, sizeof(double) * A);
    *rank = r;
    return BQ_OK;
}

namespace bqh {

// the measure of an integral call as the key of the KMEAN state (host.h, bq_fit::km_key, has the
// three layouts): the kind comes first, so that a box and a Gaussian with the same numbers differ;
// zeros behind, so that two keys compare byte by byte.  The measure has passed launch_kernel_mean.
static void kmean_key(const bq_fit *f, const Measure &m, double *key)
{
    const size_t d = (size_t)f->d;
    std::memset(key, 0, sizeof f->km_key);
    key[0] = (double)m.kind;
    switch (m.kind) {
    case Measure::GAUSS:
        std::memcpy(key + 1, m.a, sizeof(double) * d);
        std::memcpy(key + 1 + d, m.b, sizeof(double) * d * d);
        break;
    case Measure::BOX:
        std::memcpy(key + 1, m.a, sizeof(double) * d);
        std::memcpy(key + 1 + d, m.b, sizeof(double) * d);
        break;
    case Measure::MIX: {
        const size_t C = (size_t)m.C;
        key[1] = (double)C;
        std::memcpy(key + 2, m.pi, sizeof(double) * C);
        std::memcpy(key + 2 + C, m.a, sizeof(double) * d * C);
        std::memcpy(key + 2 + C + d * C, m.b, sizeof(double) * d * d * C);
        break;
    }
    }
}

static bool kmean_current(const bq_fit *f, const double *key)
{
    return (f->have & bq_fit::KMEAN) && std::memcmp(f->km_key, key, sizeof f->km_key) == 0;
}

// the measure of a warped call as the key of the SQW state: [mu d | Sigma d x d], zeros behind
static void sqw_key(const bq_fit *f, const double *mu, const double *cov, double *key)
{
    std::memset(key, 0, sizeof f->sq_key);
    std::memcpy(key, mu, sizeof(double) * f->d);
    std::memcpy(key + f->d, cov, sizeof(double) * f->d * f->d);
}

// every buffer the producer touches, there before its first launch
static int kmean_alloc(bq_ctx *c, bq_fit *f, const Measure &m)
{
    BQCHK(fit_grow(c, f->wide, sizeof(double) * wide_alloc_doubles(f->npad), "wide block inverses"));
    BQCHK(fit_vec(c, f));
    BQCHK(fit_grow(c, f->wz, sizeof(double) * (size_t)f->npad, "contiguous z"));
    if (m.kind == Measure::MIX) {
        const size_t len = mix_form_doubles(f->d, BQ_MEASURE_MAX_COMP);
        BQCHK(fit_grow(c, f->kmform, sizeof(double) * len, "mixture forms"));
        f->km_hform.resize(len);
    }
    return fit_grow(c, f->kmean, sizeof(double) * (2 * (size_t)f->npad + 32), "kernel mean state");
}

// The producer of KMEAN, first half: its launches, nothing read back.  A mixture's forms go to the
// device first; kappa_X by the measure's kernel on the resident points (zero on the padding), a
// copy into the single-vector workspace, which the sweep consumes, b = L^-1 kappa_X by the fit's
// forward single-vector sweep, and b.b.  kk is integral_args'.  The bit is dropped first: the
// state belongs to no key until fit_kmean has the sum on the host.
static int kmean_enqueue(bq_ctx *c, bq_fit *f, const Measure &m, double kk)
{
    const int npad = f->npad;
    double *kap = f->kmean.d(), *b = kap + npad, *scal = b + npad;
    f->drop(bq_fit::KMEAN);
    WideInv w;
    BQCHK(fit_wide(c, f, w));
    HIPCHK(c, hipMemsetAsync(kap, 0, sizeof(double) * (size_t)npad, c->stream));
    if (m.kind == Measure::MIX) {
        mix_forms(f->d, f->w, m, f->km_hform.data());
        HIPCHK(c, hipMemcpyAsync(f->kmform.p, f->km_hform.data(),
                                 sizeof(double) * mix_form_doubles(f->d, (int)m.C),
                                 hipMemcpyHostToDevice, c->stream));
    }
    BQCHK(launch_kernel_mean(c, f->d, f->pts.d(), f->n, f->h, f->w, m, kap, nullptr,
                             f->kmform.d()));
    f->km_kk = kk;
    BQCHK(launch_gather_row(c, f->vec.d(), kap, 1, npad));
    BQCHK(enqueue_forward_vec(c, f->vec.d(), b, f->A.d(), f->ldl, npad, w,
                              f->vec.d() + 2 * (size_t)npad));
    return launch_zd_dot(c, b, b, npad, scal);
}

// ... second half, once the stream is synchronised and b.b is on the host
static void fit_kmean(bq_fit *f, const double *key, double bb)
{
    std::memcpy(f->km_key, key, sizeof f->km_key);
    f->km_bb = bb;
    f->have |= bq_fit::KMEAN;
}

// What the integral and the design entry points check alike: the handle and the measure, before
// anything is allocated.  Leaves the measure's key, whether the KMEAN state has to be computed for
// it, and kk -- the state's where it is current (its measure passed this check before), else from
// the measure, with the factors that only kk needs.
static int integral_args(bq_ctx *c, bq_fit *f, const Measure &m, double *key, bool *fresh,
                         double *kk)
{
    BQCHK(check_fit(c, f));
    BQCHK(launch_kernel_mean(c, f->d, nullptr, 0, f->h, f->w, m, nullptr, nullptr));
    kmean_key(f, m, key);
    *fresh = !kmean_current(f, key);
    if (!*fresh) {
        *kk = f->km_kk;
        return BQ_OK;
    }
    return launch_kernel_mean(c, f->d, nullptr, 0, f->h, f->w, m, nullptr, kk);
}

// The integral of the fit under a measure (include/bqhip.h has the contracts): the body of
// bq_gp_integral and its _box and _mix twins.  Where the KMEAN state is not there for this measure
// its producer is enqueued in front; then b.z against the current z, for the weights one backward
// single-vector sweep from a copy of b, and one read-back of the two sums (and the weights).
static int gp_integral(bq_ctx *c, bq_fit *f, const Measure &m, double *mean, double *var,
                       double *weights)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    double key[bq_fit::KM_KEY_LEN];
    bool fresh;
    double kk;
    BQCHK(integral_args(c, f, m, key, &fresh, &kk));
    if (!mean && !var && !weights)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    BQCHK(kmean_alloc(c, f, m));
    const int n = f->n, npad = f->npad;
    double *b = f->kmean.d() + npad, *scal = b + npad;
    double *hs, *ds;
    BQCHK(ctx_stage(c, 2, &hs, &ds));
    BQCHK(with_flow_fallback(c, [&]() -> int {
        if (fresh)
            BQCHK(kmean_enqueue(c, f, m, kk));
        BQCHK(fit_zc(c, f));
        BQCHK(launch_zd_dot(c, b, f->wz.d(), npad, scal + 1));
        if (weights) {
            WideInv w;
            BQCHK(fit_wide(c, f, w));
            BQCHK(launch_gather_row(c, f->vec.d(), b, 1, npad));
            BQCHK(enqueue_backward_vec(c, f->vec.d(), f->vec.d() + npad, f->A.d(), f->ldl, npad, w,
                                       f->vec.d() + 2 * (size_t)npad));
            HIPCHK(c, hipMemcpyAsync(f->hvec, f->vec.d() + npad, sizeof(double) * n,
                                     hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(hs, scal, sizeof(double) * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BQ_OK;
    }));
    if (fresh)
        fit_kmean(f, key, hs[0]);
    if (mean)
        *mean = hs[1];
    if (var)
        *var = f->km_kk - f->km_bb;
    if (weights)
        std::memcpy(weights, f->hvec, sizeof(double) * n);
    return BQ_OK;
}

} // namespace bqh

extern "C" int bq_gp_integral(bq_ctx *c, bq_fit *f, const double *mu, const double *cov,
                              double *mean, double *var, double *weights)
{
    return gp_integral(c, f, Measure::gauss(mu, cov), mean, var, weights);
}

extern "C" int bq_gp_integral_box(bq_ctx *c, bq_fit *f, const double *lo, const double *hi,
                                  double *mean, double *var, double *weights)
{
    return gp_integral(c, f, Measure::box(lo, hi), mean, var, weights);
}

extern "C" int bq_gp_integral_mix(bq_ctx *c, bq_fit *f, int64_t C, const double *pi,
                                  const double *mu, const double *cov, double *mean, double *var,
                                  double *weights)
{
    return gp_integral(c, f, Measure::mix(C, pi, mu, cov), mean, var, weights);
}

namespace bqh {

// The marginal of the fit under a Gaussian or a box (include/bqhip.h has the contract; marginal.h
// the kernels): the body of bq_gp_marginal and bq_gp_marginal_box, a posterior call whose cross
// rows are partial kernel means.  Mean alone: alpha and one fused launch.  Otherwise
// bq_gp_predict's staging, forward sweep and row reductions over the marginal's own right-hand
// sides, the prior's diagonal added to -|v|^2 by its producer, and for cov the prior as the seed of
// posterior_sigma's product.  A box's column factors kappa_box,I(X) live behind the results in
// f->wout for the length of the call: no state is kept.
static int gp_marginal(bq_ctx *c, bq_fit *f, const int32_t *keep, const Measure &m,
                       const double *xq, int64_t M, double *mean, double *var, double *cov)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    BQCHK(check_fit(c, f));
    if (M < 0 || M > INT32_MAX - 64 || (M && !xq) || (!mean && !var && !cov))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    MargPlan pl;
    BQCHK(marginal_plan(c, f->d, f->h, f->w, keep, m, xq, M, &pl));
    if (M == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const int n = f->n, npad = f->npad, Mp = (int)roundup(M, 64);
    const bool sweep = var || cov;
    if (!sweep)
        BQCHK(fit_alpha(c, f));
    BQCHK(fit_grow(c, f->wout, sizeof(double) * (2 * (size_t)Mp + npad), "prediction results"));
    PosteriorIO io;
    BQCHK(io.begin(c, f, xq, M, 0, false));
    double *colv = f->wout.d() + 2 * (size_t)Mp;
    if (pl.box)
        BQCHK(launch_marginal_colv(c, pl, f->pts.d(), n, colv));
    if (!sweep) {
        BQCHK(launch_marginal_mean(c, pl, io.xq, (int)M, f->pts.d(), n, colv, f->alpha.d(), io.res));
        return io.finish(c, (size_t)Mp, mean, nullptr, nullptr, nullptr);
    }
    WideInv wi;
    BQCHK(fit_wide(c, f, wi));
    DevBuf &V0 = f->wV, &V = f->wV2;
    BQCHK(fit_grow(c, V0, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
    BQCHK(fit_grow(c, V, sizeof(double) * (size_t)Mp * npad, "prediction sweep workspace"));
    BQCHK(launch_marginal_cross(c, pl, io.xq, (int)M, Mp, f->pts.d(), n, npad, colv, V0.d(), Mp));
    BQCHK(enqueue_forward_rows(c, V0.d(), V.d(), Mp, Mp, f->A.d(), f->ldl, npad, wi));
    BQCHK(fit_zc(c, f));
    BQCHK(launch_rowdot(c, V.d(), (long)Mp, (int)M, Mp, npad, f->wz.d(), 0.0, io.res, io.res + Mp, 1));
    DevBuf Cd; // (lives until finish has synchronised the stream: one read-back)
    if (cov) {
        HIPCHK(c, Cd.alloc(sizeof(double) * (size_t)Mp * Mp));
        BQCHK(launch_marginal_prior(c, pl, io.xq, (int)M, Mp, Cd.d(), Mp, io.res + Mp, 1));
        GemmJob vvt;
        vvt.C = Cd.d(), vvt.ldc = Mp;
        vvt.P = V.d(), vvt.ldp = Mp;
        vvt.Q = V.d(), vvt.qsj = 1, vvt.qsk = Mp;
        vvt.m = Mp, vvt.n = Mp, vvt.k = npad;
        BQCHK(launch_gemm(c, BQ_K_GEMM, vvt));
        HIPCHK(c, hipMemcpy2DAsync(cov, sizeof(double) * M, Cd.p, sizeof(double) * Mp,
                                   sizeof(double) * M, M, hipMemcpyDeviceToHost, c->stream));
    } else {
        BQCHK(launch_marginal_prior(c, pl, io.xq, (int)M, Mp, nullptr, 0, io.res + Mp, 1));
    }
    return io.finish(c, 2 * (size_t)Mp, mean, var, nullptr, nullptr); // [mean | var], one copy
}

} // namespace bqh

extern "C" int bq_gp_marginal(bq_ctx *c, bq_fit *f, const int32_t *keep, const double *mu,
                              const double *cov, const double *xq, int64_t M, double *mean,
                              double *var, double *cov_out)
{
    return gp_marginal(c, f, keep, Measure::gauss(mu, cov), xq, M, mean, var, cov_out);
}

extern "C" int bq_gp_marginal_box(bq_ctx *c, bq_fit *f, const int32_t *keep, const double *lo,
                                  const double *hi, const double *xq, int64_t M, double *mean,
                                  double *var, double *cov_out)
{
    return gp_marginal(c, f, keep, Measure::box(lo, hi), xq, M, mean, var, cov_out);
}

namespace bqh {

// what the two design entry points check alike, after the measure
static int zd_args(bq_ctx *c, const double *xc, int64_t A, int64_t q, double nugget, double tol,
                   const int64_t *piv, const double *gain, const double *zvar0, const int64_t *rank)
{
    if (A < 0 || q < 1 || (A && q > A) || A > BQ_PIVCHOL_MAX_M || q > BQ_PIVCHOL_MAX_Q ||
        !(nugget >= 0.0) || !(tol >= 0.0) || !std::isfinite(nugget) || !std::isfinite(tol) ||
        !piv || !gain || !zvar0 || !rank || (A && !xc))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    return BQ_OK;
}

// every device buffer of a design's steps: their own, the prediction's with q more columns
static int zd_alloc(bq_ctx *c, bq_fit *f, const ZdPlan &pl)
{
    const size_t Ap = pl.Ap, npad = pl.npad;
    BQCHK(fit_grow(c, f->zd, sizeof(double) * pl.total, "integral design workspace"));
    BQCHK(fit_grow(c, f->wV, sizeof(double) * Ap * npad, "prediction sweep workspace"));
    return fit_grow(c, f->wV2, sizeof(double) * Ap * (npad + pl.q),
                    "prediction sweep workspace and the candidates' columns");
}

// The body the designs of a linear functional Z of the fit share (zdesign.h): bq_gp_predict's
// staging and sweep with q more columns behind V in f->wV2 -- W = [V | C] is one matrix, ld Ap --,
// kap(xc on the device, out) for Cov(Z, f(xc_a)) a priori, V b by one pass over V shaped like a
// step's product (b = L^-1 of the functional's kernel means at the fit's points); then the start
// and the q steps, enqueued one after the other with nothing read back in between.  One download
// of the workspace's head (with the device word `extra` behind it, if given) into pinned staging,
// left in *head, and one synchronise.  pre() enqueues what b needs in front.
template <class Pre, class Kap>
static int zd_run(bq_ctx *c, bq_fit *f, const ZdPlan &pl, const double *xc, int64_t A,
                  double nugget, double thr, const double *b, const double *extra, Pre &&pre,
                  Kap &&kap, double **head)
{
    const int d = f->d, nq = pl.q, Ap = pl.Ap;
    double *hs, *ds;
    BQCHK(ctx_stage(c, pl.head + 1, &hs, &ds));
    double *ws = f->zd.d(), *W = f->wV2.d();
    BQCHK(with_flow_fallback(c, [&]() -> int {
        BQCHK(pre());
        // ---- mean | var at io.res, V in the first npad columns of W
        PosteriorIO io;
        BQCHK(io.begin(c, f, xc, A, 0, false));
        BQCHK(predict_sweep(c, f, io));
        // ---- the kernel means at xc; V b, u, dc and step 0's pivot; the steps
        BQCHK(kap(io.xq, ws + pl.o_kap));
        BQCHK(launch_zd_start(c, pl, ws, W, b, io.res + Ap, nugget, thr));
        for (int t = 0; t < nq; ++t)
            BQCHK(launch_zd_step(c, pl, ws, W, d, io.xq, f->g, t, nugget, thr));
        // ---- the download
        HIPCHK(c, hipMemcpyAsync(hs, ws, sizeof(double) * pl.head, hipMemcpyDeviceToHost, c->stream));
        if (extra)
            HIPCHK(c, hipMemcpyAsync(hs + pl.head, extra, sizeof(double), hipMemcpyDeviceToHost,
                                     c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BQ_OK;
    }));
    *head = hs;
    return BQ_OK;
}

// ... and what they hand out of the head
static int zd_results(bq_ctx *c, const ZdPlan &pl, const double *hs, int64_t A, int64_t *piv,
                      double *gain, double *resid_u, double *resid_c, double *score0, int64_t *rank)
{
    const int nq = pl.q, r = reinterpret_cast<const PivcholState *>(hs)->rank;
    if (r < 0 || r > nq)
        return fail(c, BQ_ERR_HIP, "zdesign: the device left rank %d of %d steps", r, nq);
    std::memcpy(gain, hs + pl.o_gain, sizeof(double) * nq);
    std::memcpy(piv, hs + pl.o_piv, sizeof(int64_t) * nq);
    if (resid_u)
        std::memcpy(resid_u, hs + pl.o_u, sizeof(double) * A);
    if (resid_c)
        std::memcpy(resid_c, hs + pl.o_dc, sizeof(double) * A);
    if (score0)
        std::memcpy(score0, hs + pl.o_score0, sizeof(double) * A);
    *rank = r;
    return BQ_OK;
}

} // namespace bqh

namespace bqh {

// The greedy design that lowers the variance of the integral the most (include/bqhip.h has the
// contracts; zdesign.h the kernels): the body of bq_gp_zdesign and its _box and _mix twins.
// zd_run with kappa at the staged candidates and b of the KMEAN state, whose producer is enqueued
// in front where it is not there for this measure (b.b then rides behind the head).  Every device
// buffer is there before the first launch.
static int gp_zdesign(bq_ctx *c, bq_fit *f, const Measure &m, const double *xc, int64_t A,
                      int64_t q, double nugget, double tol, int64_t *piv, double *gain,
                      double *zvar0, double *resid_u, double *resid_c, double *score0,
                      int64_t *rank)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    double key[bq_fit::KM_KEY_LEN];
    bool fresh;
    double kk;
    BQCHK(integral_args(c, f, m, key, &fresh, &kk));
    BQCHK(zd_args(c, xc, A, q, nugget, tol, piv, gain, zvar0, rank));
    if (A == 0) {
        BQCHK(gp_integral(c, f, m, nullptr, zvar0, nullptr));
        for (int64_t j = 0; j < q; ++j)
            piv[j] = -1, gain[j] = 0.0;
        *rank = 0;
        return BQ_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d, npad = f->npad;
    const ZdPlan pl = zd_plan((int)A, npad, (int)q);

    BQCHK(kmean_alloc(c, f, m));
    BQCHK(zd_alloc(c, f, pl));
    double *b = f->kmean.d() + npad, *scal = b + npad, *hs;
    BQCHK(zd_run(
        c, f, pl, xc, A, nugget, tol * kk, b, scal,
        [&]() -> int { return fresh ? kmean_enqueue(c, f, m, kk) : BQ_OK; },
        [&](const double *xq, double *out) -> int {
            return launch_kernel_mean(c, d, xq, (int)A, f->h, f->w, m, out, nullptr,
                                      f->kmform.d());
        },
        &hs));
    if (fresh)
        fit_kmean(f, key, hs[pl.head]);
    *zvar0 = f->km_kk - f->km_bb;
    return zd_results(c, pl, hs, A, piv, gain, resid_u, resid_c, score0, rank);
}

} // namespace bqh

extern "C" int bq_gp_zdesign(bq_ctx *c, bq_fit *f, const double *mu, const double *cov,
                             const double *xc, int64_t A, int64_t q, double nugget, double tol,
                             int64_t *piv, double *gain, double *zvar0, double *resid_u,
                             double *resid_c, double *score0, int64_t *rank)
{
    return gp_zdesign(c, f, Measure::gauss(mu, cov), xc, A, q, nugget, tol, piv, gain, zvar0,
                      resid_u, resid_c, score0, rank);
}

extern "C" int bq_gp_zdesign_box(bq_ctx *c, bq_fit *f, const double *lo, const double *hi,
                                 const double *xc, int64_t A, int64_t q, double nugget, double tol,
                                 int64_t *piv, double *gain, double *zvar0, double *resid_u,
                                 double *resid_c, double *score0, int64_t *rank)
{
    return gp_zdesign(c, f, Measure::box(lo, hi), xc, A, q, nugget, tol, piv, gain, zvar0, resid_u,
                      resid_c, score0, rank);
}

extern "C" int bq_gp_zdesign_mix(bq_ctx *c, bq_fit *f, int64_t C, const double *pi,
                                 const double *mu, const double *cov, const double *xc, int64_t A,
                                 int64_t q, double nugget, double tol, int64_t *piv, double *gain,
                                 double *zvar0, double *resid_u, double *resid_c, double *score0,
                                 int64_t *rank)
{
    return gp_zdesign(c, f, Measure::mix(C, pi, mu, cov), xc, A, q, nugget, tol, piv, gain, zvar0,
                      resid_u, resid_c, score0, rank);
}

namespace bqh {

// the places of the SQW state's parts and of its producer's scratch in f->sqw, in doubles, from
// npad and d alone (host.h, bq_fit::sqw, names them); the slices have room for every n <= npad
struct SqwPlan {
    size_t o_r, o_b, o_scal, o_tx, o_wt, o_tq, o_wq, o_tmp, o_part, total;
};
static SqwPlan sqw_plan(int npad, int d)
{
    SqwPlan p{};
    const size_t np = (size_t)npad;
    p.o_r = 0, p.o_b = np, p.o_scal = 2 * np;
    p.o_tx = p.o_scal + 32;
    p.o_wt = p.o_tx + np * 2 * d;
    p.o_tq = p.o_wt + np;
    p.o_wq = p.o_tq + np * d;
    p.o_tmp = p.o_wq + np;
    p.o_part = p.o_tmp + np;
    const size_t tiles = (np + BQ_SQ_TJ - 1) / BQ_SQ_TJ;
    p.total = p.o_part + std::min<size_t>(tiles, BQ_SQ_MAX_SLICES) * np;
    return p;
}

static bool sqw_current(const bq_fit *f, const double *key)
{
    return (f->have & bq_fit::SQW) && std::memcmp(f->sq_key, key, sizeof f->sq_key) == 0;
}

// every buffer the producer touches, there before its first launch
static int sqw_alloc(bq_ctx *c, bq_fit *f)
{
    BQCHK(fit_grow(c, f->wide, sizeof(double) * wide_alloc_doubles(f->npad), "wide block inverses"));
    BQCHK(fit_vec(c, f));
    return fit_grow(c, f->sqw, sizeof(double) * sqw_plan(f->npad, f->d).total,
                    "square-root-warped quadrature state");
}

// The producer of SQW: its launches, nothing read back.  The fit's 2 d coordinates with alpha,
// r = W(X, X) alpha by the pair sum of the fit's points against themselves (zero on the padding),
// a copy into the single-vector workspace, b_w = L^-1 r by the fit's forward single-vector sweep,
// b_w.b_w and sq = alpha.r; then the d difference coordinates of Q with alpha n(x) for weights,
// Q's row sums and qq.  ALPHA is there (the callers run fit_alpha first).  The bit is dropped
// first: the state belongs to no key until fit_sqw has the sums on the host.
static int sqw_enqueue(bq_ctx *c, bq_fit *f, const SqForms &fm)
{
    const int d = f->d, n = f->n, npad = f->npad;
    const SqwPlan p = sqw_plan(npad, d);
    double *st = f->sqw.d(), *scal = st + p.o_scal;
    f->drop(bq_fit::SQW);
    WideInv w;
    BQCHK(fit_wide(c, f, w));
    BQCHK(launch_sq_xform(c, d, true, f->pts.d(), n, npad, fm, f->alpha.d(), st + p.o_tx,
                          st + p.o_wt));
    BQCHK(launch_sq_pair(c, d, true, st + p.o_tx, n, npad, st + p.o_tx, st + p.o_wt, n, fm.cw,
                         st + p.o_part, st + p.o_r));
    BQCHK(launch_gather_row(c, f->vec.d(), st + p.o_r, 1, npad));
    BQCHK(enqueue_forward_vec(c, f->vec.d(), st + p.o_b, f->A.d(), f->ldl, npad, w,
                              f->vec.d() + 2 * (size_t)npad));
    BQCHK(launch_zd_dot(c, st + p.o_b, st + p.o_b, npad, scal));
    BQCHK(launch_zd_dot(c, st + p.o_wt, st + p.o_r, npad, scal + 2));
    BQCHK(launch_sq_xform(c, d, false, f->pts.d(), n, npad, fm, f->alpha.d(), st + p.o_tq,
                          st + p.o_wq));
    BQCHK(launch_sq_pair(c, d, false, st + p.o_tq, n, npad, st + p.o_tq, st + p.o_wq, n, fm.cq,
                         st + p.o_part, st + p.o_tmp));
    return launch_zd_dot(c, st + p.o_wq, st + p.o_tmp, npad, scal + 1);
}

// The SQW state for this key: there already, or its producer and one read-back of the three sums
static int fit_sqw(bq_ctx *c, bq_fit *f, const SqForms &fm, const double *key)
{
    if (sqw_current(f, key))
        return BQ_OK;
    BQCHK(fit_alpha(c, f));
    double *hs, *ds;
    BQCHK(ctx_stage(c, 3, &hs, &ds));
    BQCHK(with_flow_fallback(c, [&]() -> int {
        BQCHK(sqw_enqueue(c, f, fm));
        HIPCHK(c, hipMemcpyAsync(hs, f->sqw.d() + sqw_plan(f->npad, f->d).o_scal,
                                 sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BQ_OK;
    }));
    std::memcpy(f->sq_key, key, sizeof f->sq_key);
    f->sq_bb = hs[0], f->sq_qq = hs[1], f->sq_sq = hs[2];
    f->have |= bq_fit::SQW;
    return BQ_OK;
}

// what the two warped entry points check alike: the handle, the measure, its forms
static int sq_args(bq_ctx *c, bq_fit *f, const double *mu, const double *cov, SqForms *fm)
{
    BQCHK(check_fit(c, f));
    BQCHK(launch_kernel_mean(c, f->d, nullptr, 0, f->h, f->w, Measure::gauss(mu, cov), nullptr,
                             nullptr));
    return sq_forms(c, f->d, f->h, f->w, mu, cov, fm);
}

} // namespace bqh

// Square-root-warped quadrature of the fit under N(mu, Sigma) (include/bqhip.h has the contract).
// Where the SQW state is not there for this measure its producer runs; the outputs are the
// state's own.
extern "C" int bq_gp_sqintegral(bq_ctx *c, bq_fit *f, const double *mu, const double *cov,
                                double *sq, double *var, double *r)
{
    SqForms fm;
    BQCHK(sq_args(c, f, mu, cov, &fm));
    if (!sq && !var && !r)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    HIPCHK(c, hipSetDevice(c->device));
    BQCHK(sqw_alloc(c, f));
    double key[sizeof f->sq_key / sizeof(double)];
    sqw_key(f, mu, cov, key);
    BQCHK(fit_sqw(c, f, fm, key));
    if (r) {
        HIPCHK(c, hipMemcpyAsync(f->hvec, f->sqw.d() + sqw_plan(f->npad, f->d).o_r,
                                 sizeof(double) * f->n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::memcpy(r, f->hvec, sizeof(double) * f->n);
    }
    if (sq)
        *sq = f->sq_sq;
    if (var)
        *var = f->sq_qq - f->sq_bb;
    return BQ_OK;
}

// The greedy design that lowers the variance of the warped integral the most (include/bqhip.h has
// the contract): zd_run with the pair sum of the staged candidates against the fit's transformed
// points for the kernel means and b_w of the SQW state, which is computed first where it is not
// there (qq scales the stop level, so it has to be on the host before the steps are enqueued).
// Every device buffer is there before the first launch.
extern "C" int bq_gp_sqdesign(bq_ctx *c, bq_fit *f, const double *mu, const double *cov,
                              const double *xc, int64_t A, int64_t q, double nugget, double tol,
                              int64_t *piv, double *gain, double *zvar0, double *resid_u,
                              double *resid_c, double *score0, int64_t *rank)
{
    SqForms fm;
    BQCHK(sq_args(c, f, mu, cov, &fm));
    BQCHK(zd_args(c, xc, A, q, nugget, tol, piv, gain, zvar0, rank));
    if (A == 0) {
        BQCHK(bq_gp_sqintegral(c, f, mu, cov, nullptr, zvar0, nullptr));
        for (int64_t j = 0; j < q; ++j)
            piv[j] = -1, gain[j] = 0.0;
        *rank = 0;
        return BQ_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int d = f->d, n = f->n, npad = f->npad;
    const ZdPlan pl = zd_plan((int)A, npad, (int)q);
    const size_t Ap = pl.Ap;

    BQCHK(sqw_alloc(c, f));
    BQCHK(zd_alloc(c, f, pl));
    BQCHK(fit_grow(c, f->sqc, sizeof(double) * Ap * (2 * (size_t)d + sq_pair_plan(pl.Ap, n).nsl),
                   "candidates' coordinates and pair sums"));
    BQCHK(fit_grow(c, f->wx, sizeof(double) * (size_t)d * A, "prediction points"));
    BQCHK(fit_grow(c, f->wout, sizeof(double) * 2 * Ap, "prediction results"));
    BQCHK(fit_grow(c, f->wz, sizeof(double) * (size_t)npad, "contiguous z"));
    double key[sizeof f->sq_key / sizeof(double)];
    sqw_key(f, mu, cov, key);
    BQCHK(fit_sqw(c, f, fm, key));
    const SqwPlan sp = sqw_plan(npad, d);
    const double *st = f->sqw.d();
    double *tp = f->sqc.d(), *part = tp + Ap * 2 * d, *hs;
    BQCHK(zd_run(
        c, f, pl, xc, A, nugget, tol * f->sq_qq, st + sp.o_b, nullptr,
        []() -> int { return BQ_OK; },
        [&](const double *xq, double *out) -> int {
            BQCHK(launch_sq_xform(c, d, true, xq, (int)A, (int)A, fm, nullptr, tp, nullptr));
            return launch_sq_pair(c, d, true, tp, (int)A, pl.Ap, st + sp.o_tx, st + sp.o_wt, n,
                                  fm.cw, part, out);
        },
        &hs));
    *zvar0 = f->sq_qq - f->sq_bb;
    return zd_results(c, pl, hs, A, piv, gain, resid_u, resid_c, score0, rank);
}

