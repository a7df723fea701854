// host.h -- internal header of libbqhip.so's host side: the context, the handle types and
// the launch / enqueue helpers the translation units share.  Nothing here is part of the C
// ABI (include/bqhip.h is); the library is built with hidden visibility and exports only
// the extern "C" entry points.  The switches that select launches and the hipGraph a launch sequence
// is captured into live in launch_config.h (LaunchConfig: one list; CapturedSeq: the only code that
// captures, launches or destroys a graph); bq_ctx::cfg is the former, plans, pairs and fits hold the
// latter.
//
// Translation units (Makefile; all but probe.hip make libbqhip.so, all of them together
// libbqhip_probe.so, whose extra entry points include/bqhip_probe.h declares):
//   k_gram.hip   gram.h kernels                 launch_gram_sym / _cross
//   k_gemm.hip   gemm.h trsmsweep.h kernels     launch_gemm, launch_gemm_rows, launch_rows_step
//   k_hess.hip   hess.h loo.h lgo.h kernels     the log-ML Hessian's sums, leave-one-out and
//                                               leave-group-out
//                ptheta.h kernels               the posterior's derivatives in the hyper-parameters
//                dk.h wgsum.h                   (shared: the derivative operand's entries and D_k a
//                                               rows; a workgroup's fixed-order sums, fold_kernel)
//   k_panel.hip  potf2.h trsm.h slab.h kernels  launch_assemble, launch_potf2, launch_trsm_blk,
//                                               the one-launch steps
//                solve16.h                      (both units: the 16-row solve from block inverses,
//                                               its fragment loaders and LDS staging)
//   k_reduce.hip reduce.h trsv.h append.h        read-outs, single-vector sweeps, utilities, the
//                remove.h kernels               finishing kernels of an append, shrinking a fit
//                pgrad.h kernels                the posterior's gradients at the query points
//                sample.h kernels               the posterior samples' normals and triangular product
//                pivchol.h kernels              the pivoted partial Cholesky of a posterior
//                ivr.h kernels                  designs that minimise the integrated variance
//                zdesign.h kernels              the integral of a fit, designs that lower its variance
//                sqwarp.h kernels               the pair sums of square-root-warped quadrature
//                trend.h kernels                the polynomial trend of a fit, marginalised
//   potrf.hip    the sweep route (sweep_route), the blocked factorisation's launch sequences
//                and the bordered pass of plans and fits (no kernels of its own)
//   sweeps.hip   sweeps over a resident factor (no kernels of its own)
//   ctx.hip      contexts, device memory, timers, the launch profiler
//   linalg.hip   linalg_c drop-ins, Gram entry points, bq_potrf_dev
//   plan.hip     resident batched plans, batched / grid entry points
//   fit.hip      resident GP fits
//   moments.hip  closed-form integrals, BQ moments, the acquisition entry points
//                marginal.h kernels             the marginal of a fit: partial kernel means, its prior
//   pair.hip     the stacked pair of GPs at S hyper-parameter sets in one batched pass
//   probe.hip    hardware probes (libbqhip_probe.so only)
#pragma once
#include <hip/hip_runtime.h>

#pragma GCC visibility push(default)
#include "../../include/bqhip.h"
#pragma GCC visibility pop

#include "launch_config.h"
#include "types.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

// Guard bands (tests): with bq_set_guard(1) every device buffer allocated afterwards carries
// BQ_GUARD_BYTES of 0xA5 behind its last byte; bq_plan_check_guards counts the bytes of a plan's
// bands that a pass has overwritten (round 5 found a workspace sized for the wrong block width
// only because the next allocation happened to fault).
#define BQ_GUARD_BYTES 4096
inline bool &devbuf_guard()
{
    static bool on = std::getenv("BQ_GUARD") && std::atoi(std::getenv("BQ_GUARD"));
    return on;
}

// RAII device buffer
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    size_t guard = 0; // bytes of sentinel behind `bytes` (0: none)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        guard = 0;
    }
    hipError_t alloc(size_t b)
    {
        release();
        if (b == 0)
            b = 8;
        const size_t g = devbuf_guard() ? BQ_GUARD_BYTES : 0;
        hipError_t e = hipMalloc(&p, b + g);
        if (e == hipSuccess && g)
            e = hipMemset(static_cast<char *>(p) + b, 0xA5, g);
        if (e == hipSuccess) {
            bytes = b;
            guard = g;
        } else {
            if (p)
                (void)hipFree(p);
            p = nullptr;
        }
        return e;
    }
    // bytes of the guard band that no longer hold the sentinel (-1: the read failed)
    long guard_damage() const
    {
        if (!p || !guard)
            return 0;
        unsigned char h[BQ_GUARD_BYTES];
        if (hipMemcpy(h, static_cast<const char *>(p) + bytes, guard, hipMemcpyDeviceToHost) != hipSuccess)
            return -1;
        long bad = 0;
        for (size_t i = 0; i < guard; ++i)
            bad += h[i] != 0xA5;
        return bad;
    }
    void swap(DevBuf &o)
    {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        std::swap(guard, o.guard);
    }
    double *d() const { return static_cast<double *>(p); }
    int *i() const { return static_cast<int *>(p); }
};

struct ProfEvent {
    hipEvent_t a, b;
    int cls;
    double work;
    int on_aux; // recorded on the context's second stream
};

struct bq_ctx {
    int device = 0;
    hipStream_t stream = nullptr; // main stream: everything is ordered on it
    hipStream_t aux = nullptr;    // high-priority panel stream of the look-ahead Cholesky
    hipStream_t cur = nullptr;    // stream the launch helpers enqueue on (stream or aux)
    hipEvent_t ev_panel = nullptr, ev_next = nullptr, ev_fork = nullptr, ev_top = nullptr;
    LaunchConfig cfg;    // every field an environment switch or a setter writes (launch_config.h)
    CaptureStats graphs; // what the captured sequences of this context did (bq_ctx_stats)
    int *flow_abort = nullptr; // mapped host word a timed-out hand-off raises
    long n_flow_fallback = 0;  // solves re-issued on the per-block sweeps after such a time-out
                               // (bq_ctx_stats)
    double *hstage = nullptr; // mapped pinned staging of the small host-buffer calls (ctx_stage)
    size_t hstage_len = 0;
    DevBuf panel_ws;     // scratch panel columns of the eager linalg entry points
    DevBuf scratch;      // per-call temporaries of the acquisition / moment entry points, kept
                         // between calls (hipFree synchronises the device); bq_ctx_trim frees it
    int sharing = 0;     // how the chip is shared while the launches being queued run (gemm_route):
                         // 0 alone, 1 the two streams of a look-ahead, 2 the two halves of a batch
    bool own_stream = false;
    int cus = 256;
    bq_plan *plan_cache = nullptr; // workspace of the last batched call, kept for the next one
    char err[512] = {0};
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool prof = false;
    std::vector<ProfEvent> prof_events;
    // bq_profile_timeline: (class, stream, start, end in ms since the first bracket) per launch
    bool prof_keep_timeline = false;
    hipEvent_t prof_origin = nullptr;
    std::vector<double> prof_timeline;
    double prof_ms[BQ_K_NCLASS] = {0};
    int64_t prof_n[BQ_K_NCLASS] = {0};
    double prof_work[BQ_K_NCLASS] = {0};
    DevBuf gbuf;   // GaussParams of the single-problem entry points (cached)
    GaussParams gbuf_host{};
    bool gbuf_valid = false;
    DevBuf dinv64; // potf2 reciprocal-diagonal scratch
    bool remove_lds_set = false; // remove_diag_kernel's dynamic LDS limit is raised (launch_remove_step)
};

namespace bqh {

inline int fail(bq_ctx *c, int code, const char *fmt, ...)
{
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof c->err, fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIPCHK(c, call)                                                                        \
    do {                                                                                       \
        hipError_t e__ = (call);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return bqh::fail((c), e__ == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP,      \
                             "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, \
                             __LINE__);                                                        \
    } while (0)

#define BQCHK(call)                                                                            \
    do {                                                                                       \
        int s__ = (call);                                                                      \
        if (s__ != BQ_OK)                                                                      \
            return s__;                                                                        \
    } while (0)

inline long roundup(long v, long q) { return (v + q - 1) / q * q; }

// The one switch on the dimension: the statement(s) after d_ with `constexpr int D` bound to it,
// once per template instantiation D = 1 .. 8 (anything else takes 8: callers check d first)
#define BQ_DISPATCH_D(d_, ...)                                                                     \
    switch (d_) {                                                                                  \
    case 1: { constexpr int D = 1; __VA_ARGS__; } break;                                           \
    case 2: { constexpr int D = 2; __VA_ARGS__; } break;                                           \
    case 3: { constexpr int D = 3; __VA_ARGS__; } break;                                           \
    case 4: { constexpr int D = 4; __VA_ARGS__; } break;                                           \
    case 5: { constexpr int D = 5; __VA_ARGS__; } break;                                           \
    case 6: { constexpr int D = 6; __VA_ARGS__; } break;                                           \
    case 7: { constexpr int D = 7; __VA_ARGS__; } break;                                           \
    default: { constexpr int D = 8; __VA_ARGS__; } break;                                          \
    }

// leading dimension for an ntot x ntot column-major matrix: even, and nudged
// off large powers of two so that the 4 columns of an MFMA fragment do not
// all map to the same HBM channel / L2 set
inline long pick_ld(long ntot)
{
    long ld = ntot;
    if (ntot >= 1024 && (ntot % 512) == 0)
        ld += 64;
    return ld;
}

inline GaussParams make_params(int d, double h, const double *w, double s)
{
    GaussParams g;
    std::memset(&g, 0, sizeof g);
    double c = h * h;
    for (int k = 0; k < d; ++k) {
        c /= (std::sqrt(2.0 * M_PI) * w[k]);
        g.nh[k] = -0.5 / (w[k] * w[k]);
    }
    g.c = c;
    g.s2 = s * s;
    return g;
}

inline Layout make_layout(int n, int M, bool has_y)
{
    Layout L;
    L.n = n;
    L.npad = (int)roundup(n, 64);
    L.M = M;
    L.yrow = has_y ? L.npad + M : -1;
    L.ntot = (int)roundup(L.npad + M + (has_y ? 1 : 0), 64);
    return L;
}

// ---- profiling brackets: HIP events around a launch, on the stream it goes to ----
struct Bracket {
    bq_ctx *c;
    ProfEvent ev;
    bool on;
    Bracket(bq_ctx *ctx, int cls, double work = 0.0) : c(ctx), on(ctx->prof)
    {
        if (on) {
            ev.cls = cls;
            ev.work = work;
            ev.on_aux = ctx->cur != ctx->stream;
            if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) {
                on = false;
                return;
            }
            (void)hipEventRecord(ev.a, c->cur);
        }
    }
    ~Bracket()
    {
        if (on) {
            (void)hipEventRecord(ev.b, c->cur);
            c->prof_events.push_back(ev);
        }
    }
};

int prof_collect(bq_ctx *c); // ctx.hip

// Carves the per-call temporaries of one entry point out of the context's scratch buffer:
// sizes first (take), then one commit that grows the buffer if it must, then the pointers.
struct Scratch {
    bq_ctx *c;
    size_t total = 0;
    explicit Scratch(bq_ctx *ctx) : c(ctx) {}
    size_t take(size_t doubles)
    {
        const size_t off = total;
        total += (doubles + 31) & ~(size_t)31; // 256-byte granules
        return off;
    }
    int commit()
    {
        if (c->scratch.bytes < total * sizeof(double)) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, c->scratch.alloc(total * sizeof(double)));
        }
        return BQ_OK;
    }
    double *at(size_t off) const { return c->scratch.d() + off; }
};

int check_dims(bq_ctx *c, int64_t d, int64_t n);                          // ctx.hip
int check_w(bq_ctx *c, int64_t d, double h, const double *w, double s);   // ctx.hip

// ---- k_gram.hip -----------------------------------------------------------------------
int launch_gram_sym(bq_ctx *c, int d, const double *x, long xstride, const GaussParams *gp,
                    int gpstride, double *K, long ldk, long kstride, int n, int batch);
int launch_gram_cross(bq_ctx *c, int d, const double *x1, int n1, const double *x2, int n2,
                      const GaussParams &g, double *K, long ldk);
int launch_gram_cross_pad(bq_ctx *c, int d, const double *x1, int n1, int n1p, const double *x2,
                          int n2, int n2p, const GaussParams &g, double *K, long ldk);

// ---- k_panel.hip ----------------------------------------------------------------------
// fs: when set, the first launch of the slab sweep rides in the assembly (assemble_first_kernel)
struct FirstStep {
    double *S0 = nullptr;
    long lds = 0, sstride = 0;
    double *dinv = nullptr;
    int *info = nullptr;
    double *scal = nullptr; // SlabOut::scal: log|K| starts here (the leading block's factor stores it)
    long long *stamps = nullptr; // the profiling instantiation (bq_probe_first_launch), d = 1
};
// jcols > 0: only the first jcols columns (a multiple of 64) of every system
int launch_assemble(bq_ctx *c, int d, const double *pts, long pstride, const double *y,
                    long ystride, const GaussParams *gp, int gpstride, double *A, long lda,
                    long astride, Layout L, int batch, const FirstStep &fs = FirstStep(),
                    int jcols = 0);
// rows [sd.r, sd.r + m) x columns [sd.c, sd.c + n) of the systems sd describes (lower part)
int launch_assemble_region(bq_ctx *c, const GramSeed &sd, double *A, long lda, long astride, int m,
                           int n, int batch);
int launch_potf2(bq_ctx *c, double *A, long lda, long astride, int j0, double *dinv, long dstride,
                 int *info, int batch);
int launch_potrf_wg(bq_ctx *c, double *A, long lda, long astride, int kb, double *rec, long rstride,
                    int *info, int col0, int batch);
int launch_trsm_blk(bq_ctx *c, double *X, long ldx, long xstride, int m, const double *L11,
                    long ldl, long lstride, const double *dinv, long dstride, int batch);
// the 16 x 16 block inverses of every 64 x 64 diagonal block of a factor (npad / 64 records)
int launch_diag_winv(bq_ctx *c, const double *L, long ldl, int npad, double *dw);
int launch_panel_step(bq_ctx *c, double *A, long lda, long astride, int batch, int nrb,
                      double *Sin, double *Sout, long lds, long sstride, int K0, int j0,
                      double *dinv_in, double *dinv_out, int has_next, int first, double *SL,
                      int *info, double work);
int launch_slab_first(bq_ctx *c, double *A, long lda, long astride, int batch, double *S, long lds,
                      long sstride, int ntot, double *dinv, int *info, int col0,
                      long dstride = BQ_DINV_STRIDE);
int launch_slab_step(bq_ctx *c, double *A, long lda, long astride, int batch, double *Sin,
                     double *Sout, long lds, long sstride, int ntot, int j0, double *dinv_in,
                     double *dinv_out, int fnext, int last, int *info, int col0,
                     const SlabOut &out, long long *stamps, double work,
                     long dstride = BQ_DINV_STRIDE);

// ---- k_gemm.hip -----------------------------------------------------------------------
int gemm_init(bq_ctx *c); // function attributes of the LDS-staged kernels, once per context
// the log-ML gradient's product and finalize (gemm_lds_grad_kernel, fold_kernel<GradScale>)
int grad_tile(const bq_ctx *c, int npad); // 128 / 64: its workgroup tile (the Hessian's follows it)
size_t grad_parts(int npad, int d);
int launch_logml_grad(bq_ctx *c, int d, const double *Y, int npad, const GradJob &gj,
                      const GradScale &sc, double *grad);
// ---- k_hess.hip ----------------------------------------------------------------------
// the log-ML Hessian (hess.h) in two stages over one workspace (hess_ws_doubles).  The products
// stage: Ki = Y Y^T, B_k = Ki D_k, V = D_p a, Z = Ki V (fit_prod runs it; leave-one-out and
// leave-group-out read it too) ...
size_t hess_ws_doubles(int npad, int d);
int launch_hess_products(bq_ctx *c, int d, const double *Y, double *Ki, double *ws,
                         const HessJob &hj, const double *y, double h, double s);
// ... and the sums over what it left in Ki and ws; *sums: where they are on the device
int launch_hess_sums(bq_ctx *c, int d, const double *Ki, double *ws, const HessJob &hj,
                     const double **sums);
// out[c] = the sum over i < nitem of part[i item_stride + c c_stride], c < nc, a workgroup per c
// (fold_kernel<FoldPlain>, wgsum.h: the unit's one instantiation serves the others' partial sums)
void launch_fold(bq_ctx *c, const double *part, int nitem, long item_stride, long c_stride, int nc,
                 double *out);
// leave-one-out (loo.h) into its own workspace; *vecs: mu | var | lp, npad apart
size_t loo_ws_doubles(int npad, int d);
int launch_loo(bq_ctx *c, int d, const double *Y, const double *alpha, const double *y, int n,
               int npad, double *ws, const double **vecs, const double **total);
int launch_loo_grad(bq_ctx *c, int d, const double *Ki, const double *hws, const double *alpha,
                    int n, int npad, double h, double s, double s2, double *ws, const double **grad);
// leave-group-out (lgo.h) into its own workspace: G groups of T members in all, packed into NB
// bundles of consecutive groups with at most 64 members together (group bundle[q] begins bundle
// q).  The views of one workspace (lgo_ws_doubles; with grad: the partials of Q_BB and the M_k
// behind the rest)
struct LgoWs {
    int *idx, *start, *flag;      // T, G + 1, 1
    int *bundle;                  // NB + 1 <= G + 1
    double *sig, *r, *mu, *var;   // T x 64, T, T, T
    double *lp, *ar, *gpart, *out; // G, G, G (d + 2), total | grad
    double *part;                 // [nchunk][T][64]; with grad [1 + d][nchunk][T][64] follow
};
size_t lgo_ws_doubles(int npad, int d, long T, long G, bool grad);
LgoWs lgo_views(double *ws, int npad, int d, long T, long G);
// maxb: the largest bundle.  launch_lgo: mu, var, lp, total (*out) and what the gradient reads
int launch_lgo(bq_ctx *c, const double *Y, const double *alpha, const double *y, int n, int npad,
               int d, long T, long G, long NB, int maxb, const LgoWs &w);
// after launch_lgo on the same workspace: the gradient (out + 1) from the products stage (Ki, hws)
int launch_lgo_grad(bq_ctx *c, int d, const double *Ki, const double *hws, int n, int npad, long T,
                    long G, long NB, int maxb, double h, double s, double s2, const LgoWs &w);
// the posterior's derivatives in the hyper-parameters (ptheta.h): the right-hand sides of the fit's
// solved vectors, q_jk = beta_j^T D_k beta_j in column-block pieces (ptheta_part_doubles of them),
// the row sums with the finished derivatives, and the fused mean route
int launch_ptheta_dka(bq_ctx *c, int d, const HessJob &hj, double *R);
size_t ptheta_part_doubles(int d, int Mp, int npad);
int launch_ptheta_quad(bq_ctx *c, int d, const double *beta, long ldb, int Mp, const HessJob &hj,
                       double *part);
int launch_predict_theta(bq_ctx *c, int d, const double *beta, long ldb, int M, int Mp,
                         const double *xo, const HessJob &hj, const double *Z, const double *var,
                         const double *qpart, double h, double s, double *dmean, double *dvar);
int launch_predict_mean_theta(bq_ctx *c, int d, const double *xo, int M, const HessJob &hj,
                              const double *Z, double h, double s, double *mean, double *dmean);

// ---- k_gemm.hip (continued) -----------------------------------------------------------
// One product C(m x n) -= P(m x k) Q(n x k)^T per batch element, as operands and a shape.
struct GemmJob {
    double *C = nullptr;
    long ldc = 0, cstride = 0;
    const double *P = nullptr;
    long ldp = 0, pstride = 0;
    const double *Q = nullptr; // Q(j, k) at Q[j qsj + k qsk]
    long qsj = 0, qsk = 0, qstride = 0;
    int m = 0, n = 0, k = 0;
    int lower = 0; // only the lower trapezoid of C is needed
    int batch = 1;
    int ccut = 0;  // > 0: columns >= ccut of C need no update (honoured by the LDS-staged kernels)
    const GramSeed *seed = nullptr; // C was left out of the assembly: compute it from the points
    // request: also factor the leading 64 x 64 block of C (global column j0) in the same launch;
    // dinv / info as for launch_potf2.  Whether the launch carried it: GemmRoute::fused
    struct Fuse {
        int j0 = -1;
        double *dinv = nullptr;
        long dstride = 0;
        int *info = nullptr;
    } fuse;
    bool rows = false; // a sweep's product (one matrix, few rows, a long k): split-k tiles allowed
};
// Which kernel takes a product, decided in ONE place (gemm_route, k_gemm.hip) -- the third routing
// function beside sweep_route and rows_route.  launch_gemm asks it once and reports what it ran.
struct GemmRoute {
    // Lds128 / Lds64: gemm_lds_kernel / gemm_lds64_kernel (QT: Q k-contiguous); Sub128 / 64 / 32:
    // gemm_sub_kernel<4 | 2 | 1>; K64x64 / K64x32: gemm_k64_kernel<2 | 1>; SplitK: gemm_splitk_kernel
    enum Kernel { Lds128, Lds64, Lds64QT, Sub128, Sub64, Sub32, K64x64, K64x32, SplitK } kernel;
    int mfma;            // Sub*: 4 (the 4x4x4 four-block MFMA) or 16 (16x16x4); else 0
    dim3 grid;
    bool fused;          // the launch carries the diagonal factor GemmJob::fuse asked for
    bool seeded;         // the kernel computes its own C tile from the points (GemmJob::seed)
    bool assemble_first; // a seed was given but the kernel cannot seed: the region is assembled first
    int syrk_cls;        // profile class of a BQ_K_SYRK product: BQ_K_SYRK_SMALL below a chip of 128-tiles
};
GemmRoute gemm_route(const bq_ctx *c, const GemmJob &g);
// ran: the route the launch took
int launch_gemm(bq_ctx *c, int cls, const GemmJob &g, GemmRoute *ran = nullptr);
bool gemm_trsm_ok(const bq_ctx *c, int m, int n, int k);
int launch_gemm_trsm(bq_ctx *c, double *C, long ldc, long cstride, const double *P, long ldp,
                     long pstride, const double *Q, long ldq, long qstride, int m, int n, int k,
                     const double *Lss, long ldl, long lstride, const double *wrec, long wstride,
                     int batch);
int launch_trsm_sweep(bq_ctx *c, double *X, long ldx, long xstride, int m, const double *L11,
                      long ldl, long lstride, const double *rec, long rstride, int kb, int batch);
int launch_gemm_rows(bq_ctx *c, int cls, double *C, long ldc, const double *P, long ldp,
                     const double *Q, long qsj, long qsk, int m, int n, int k);
int launch_rows_step(bq_ctx *c, int mrows, const RowsJob &a, const RowsJob &b, double work);
int launch_rows_fused(bq_ctx *c, int mrows, const RowsJob &a, double *C, long ldc, const double *P,
                      long ldp, const double *Q, long ldq, int n, int k, bool qt, double work);

// ---- k_reduce.hip ---------------------------------------------------------------------
int launch_finalize(bq_ctx *c, const double *A, long lda, long astride, Layout L, double *scal,
                    double *mean, double *var, long mstride, int batch, double work = 0.0);
int launch_plan_readout(bq_ctx *c, const double *A, long lda, long astride, Layout L,
                        const GaussParams *gp, double *scal, double *mean, double *var,
                        long mstride, int batch);
int launch_rowdot(bq_ctx *c, const double *V, long ldv, int M, int Mp, int npad, const double *z,
                  double k0, double *mean, double *var, long zstride = 1);
int launch_predict_mean(bq_ctx *c, int d, const double *xo, int M, const double *pts, int n,
                        const double *alpha, const GaussParams &g, double *mean);
int launch_predict_grad(bq_ctx *c, int d, const double *beta, long ldb, int M, int Mp,
                        const double *xo, const double *pts, int n, const double *alpha,
                        const GaussParams &g, double *dmean, double *dvar);
int launch_predict_mean_grad(bq_ctx *c, int d, const double *xo, int M, const double *pts, int n,
                             const double *alpha, const GaussParams &g, double *mean,
                             double *dmean);
// posterior samples (sample.h): the device normals, the diagonal of the matrix to factor (add on
// its first M entries, 1 on the padding), out = mean 1^T + tril(L) Z
int launch_normal_fill(bq_ctx *c, double *Z, long ldz, int M, int Mp, int S, uint64_t seed);
int launch_sample_diag(bq_ctx *c, double *A, long lda, int M, int Mp, double add);
int launch_tri_sample(bq_ctx *c, const double *L, long ldl, const double *Z, long ldz,
                      const double *mean, double *out, long ldo, int M, int Mp, int S);
// the pivoted partial Cholesky of a posterior (pivchol.h): the shape of q steps and the places of
// the workspace's parts in doubles -- [PivcholState | gain q | piv q (int64) | d Mp], the `head`
// doubles that go back to the host, then taken (Mp ints) | the workgroups' candidates | part
// (nsl x Mp); the start (d = var at the M real rows, step 0's pivot) and step j
struct PivcholPlan {
    int rb, ks, nblk, nsl;
    size_t o_gain, o_piv, o_d, head, o_taken, o_candv, o_candi, o_part, total;
};
PivcholPlan pivchol_plan(int Mp, int npad, int q);
int launch_pivchol_init(bq_ctx *c, const PivcholPlan &pl, double *ws, const double *var, int M,
                        int Mp, int q, double thr);
int launch_pivchol_step(bq_ctx *c, const PivcholPlan &pl, double *ws, double *W, int d,
                        const double *xq, const GaussParams &g, int M, int Mp, int npad, int q,
                        int j, double nugget, double thr);
// designs that minimise the integrated posterior variance (ivr.h): A candidates (Ap rows of T,
// rows cand0 .. of the Mp-row workspace W), R reference points (Rp columns of T; self: they are the
// candidates, Rp = Ap, dr is dc).  The places of the workspace's parts in doubles --
// [PivcholState | dc[p] + nugget | sum rho dr | gain q | piv q (int64) | dc Ap | dr Rp | score0 Ap],
// the `head` doubles that go back to the host, then taken (Ap ints) | the workgroups' candidates |
// c Ap | u Rp | rho Rp | part (nsl x Ap) | the product's part (wnsl x Mp); the start and step t
struct IvrPlan {
    int A, Ap, R, Rp, Mp, cand0, npad, q;
    bool self;
    int rb, js, nsl, nblk;  // the pass over T: rows per workgroup, columns per slice, slices
    int wrb, wks, wnsl;     // pivchol_col_kernel over the candidate rows of W
    size_t o_den, o_ivar, o_gain, o_piv, o_dc, o_dr, o_score0, head, o_taken, o_candv, o_candi,
        o_c, o_u, o_rho, o_part, o_wpart, total;
};
IvrPlan ivr_plan(int A, int R, bool self, int npad, int q);
int launch_ivr_init(bq_ctx *c, const IvrPlan &pl, double *ws, const double *var);
int launch_ivr_step(bq_ctx *c, const IvrPlan &pl, double *ws, double *T, double *W, int d,
                    const double *xc, const GaussParams &g, int t, double nugget, double thr);
// the integral of a fit and the designs that lower its variance (zdesign.h): A candidates, the Ap
// rows of the workspace W = [V | C].  The places of the workspace's parts in doubles --
// [PivcholState | dc[p] + nugget, u_p | gain q | piv q (int64) | dc Ap | u Ap | score0 Ap], the
// `head` doubles that go back to the host, then taken (Ap ints) | the workgroups' candidates |
// kappa(xc) Ap | the product's part (nsl x Ap; first V b's slices); a . b over n entries; the start
// (V: the first npad columns of W; b: npad) and step t
struct ZdPlan {
    int A, Ap, npad, q;
    int rb, ks, nsl, nblk; // pivchol_plan's for Ap rows
    size_t o_den, o_gain, o_piv, o_dc, o_u, o_score0, head, o_taken, o_candv, o_candi, o_kap,
        o_part, total;
};
ZdPlan zd_plan(int A, int npad, int q);
int launch_zd_dot(bq_ctx *c, const double *a, const double *b, int n, double *out);
int launch_zd_start(bq_ctx *c, const ZdPlan &pl, double *ws, const double *W, const double *b,
                    const double *var, double nugget, double thr);
int launch_zd_step(bq_ctx *c, const ZdPlan &pl, double *ws, double *W, int d, const double *xc,
                   const GaussParams &g, int t, double nugget, double thr);
// square-root-warped quadrature of a fit (sqwarp.h): the column slices of a pair sum over ldp
// stored rows and n columns (js columns each, a multiple of BQ_SQ_TJ) from the shapes alone; a
// point set's coordinates and weights (`sums`: the 2 d coordinates of W, else the d of Q); and
// out[a] = scale sum_j pair(tp_a, tx_j) wt_j over R rows (Rp stored, zero from R on), part:
// nsl x Rp doubles
struct SqPlan {
    int nsl, js;
};
SqPlan sq_pair_plan(long ldp, int n);
int launch_sq_xform(bq_ctx *c, int d, bool sums, const double *x, int n, int np, const SqForms &f,
                    const double *alpha, double *t, double *wt);
int launch_sq_pair(bq_ctx *c, int d, bool sums, const double *tp, int R, int Rp, const double *tx,
                   const double *wt, int n, double scale, double *part, double *out);
// the polynomial trend of a fit (trend.h).  The places of the state's parts in doubles, from npad
// alone: [H, then the sweep's partial sums (64 x npad) | G = L^-1 H as rows (64 x npad) | alpha_t
// (npad) | the slices' shares of A and b (npad / 64 slices of 64 columns, the largest basis) | A, b
// | what trend_solve_kernel leaves (BQ_TREND_STATE)]
struct TrendPlan {
    int nsl;
    size_t o_H, o_G, o_alpha, o_part, o_sums, o_tr, total;
};
TrendPlan trend_plan(int npad);
// How bq_gp_predict_trend's reductions go out, decided in ONE place (trend_route): Mean, the fused
// launch without a sweep; OnePass, rowdot_trend_kernel; Gemm, launch_rowdot and one GemmJob
enum class TrendRoute { Mean = 0, OnePass = 1, Gemm = 2 };
TrendRoute trend_route(int p, bool want_var);
// phi of the d x m points x into out[k rs + j cs], zero for m <= j < mp and on rows p .. 63
int launch_trend_basis(bq_ctx *c, int d, const double *x, int m, int mp, const TrendBasis &tb,
                       double *out, long rs, long cs);
// A = G G^T (p x p) | b = G z (p) into sums, through part (TrendPlan::o_part)
int launch_trend_sums(bq_ctx *c, const double *G, const double *z, int npad, int p, double *part,
                      double *sums);
int launch_trend_solve(bq_ctx *c, const double *sums, int p, const double *G, const double *z,
                       int npad, double *tr, double *zt);
// launch_rowdot's mean and var, and R (Mp x 64, ld Mp; phi on entry) -= V G^T in its first p <=
// BQ_TREND_ONEPASS_MAXP columns
int launch_rowdot_trend(bq_ctx *c, const double *V, long ldv, int M, int Mp, int npad,
                        const double *z, double k0, const double *G, int p, double *mean,
                        double *var, double *R);
// mean += R beta, var += |L_A^-1 r|^2 over the M rows of R; status[0] = the solve's status
int launch_trend_finish(bq_ctx *c, const double *R, long ldr, int M, int p, const double *tr,
                        double *mean, double *var, double *status);
int launch_trend_mean(bq_ctx *c, int d, const double *xo, int M, const double *pts, int n,
                      const double *alpha_t, const GaussParams &g, const TrendBasis &tb,
                      const double *tr, double *mean, double *status);
int launch_neg_identity(bq_ctx *c, double *nr, int B, int npad);
int launch_pad_identity(bq_ctx *c, double *A, long lda, int n, int ntot);
int launch_logdet(bq_ctx *c, const double *diag, long stride, int n, double *out);
int launch_transpose_pad(bq_ctx *c, const double *src, long lds, int rows, int cols, double *dst,
                         long ldd);
int launch_transpose_blocks(bq_ctx *c, const double *src, double *dst, int B, long bstride,
                            int bx, int by, int batch);
int launch_neg_sumsq(bq_ctx *c, const double *v, int n, double *out);
int launch_trsv_fwd(bq_ctx *c, const double *L, long ldl, int J, int bJ, int B, int nupd,
                    const double *nr, const double *tt, double *x, double *y, double work);
int launch_trsv_bwd(bq_ctx *c, const double *L, long ldl, int J, int bJ, int B, int bn, int nupd,
                    const double *nt, const double *uu, double *x, double *y, double work);
// a whole sweep in one launch (trsvflow.h); flow_check: BQ_ERR_HIP if a hand-off of a sweep that
// has completed on the stream timed out (call after synchronising)
bool trsv_flow_ok(const bq_ctx *c, int npad, int B, bool prefilled = false);
size_t trsv_flow_ws_doubles(int npad, int B);
// preset: ws and y hold the sentinel already (launch_flow_in: the right-hand side in from a mapped
// pinned vector + every hand-off slot of both sweeps, one launch; launch_flow_out: the solution out)
int launch_trsv_flow(bq_ctx *c, bool forward, const double *L, long ldl, int npad, int B,
                     const double *m1, const double *m2, const double *x0, double *y, double *ws,
                     bool preset = false);
int launch_flow_in(bq_ctx *c, const double *hsrc, int n, double *x, int npad, double *fill,
                   size_t nfill);
int launch_flow_out(bq_ctx *c, const double *x, int n, double *hdst);
int launch_gather_row(bq_ctx *c, double *dst, const double *src, long stride, int n);
// small host matrices through the context's mapped pinned staging buffer (trsvflow.h)
int launch_mat_in(bq_ctx *c, const double *stage, int n, double *A, long lda, int ntot, int *info);
int launch_mat_out(bq_ctx *c, double *out, const double *A, long lda, int n, const int *info);
int ctx_stage(bq_ctx *c, size_t words, double **host, double **dev);
// (L L^T) X = B, n <= 64, nrhs <= 64, one launch on the staging buffer [X | L | B]
int launch_small_potrs(bq_ctx *c, double *stage, int n, int nrhs);
// a small plan's inputs out of / results into one mapped pinned staging buffer (trsvflow.h)
int launch_plan_scatter(bq_ctx *c, const double *stage, int nprob, int d, int n, int M, int ntot,
                        int npad, int gw, double *gp, double *pts, double *yd);
int launch_plan_gather(bq_ctx *c, double *out, const double *scal, const int *info,
                       const double *mean, const double *var, int nb, int M);
// up to two small copies of 8-byte words in one launch (either side may be mapped pinned memory)
int launch_copy_words2(bq_ctx *c, void *d1, const void *s1, size_t n1, void *d2, const void *s2,
                       size_t n2);
int flow_check(bq_ctx *c);
// growing a resident fit by k observations (append.h): the finishing path of k <= 64, the pieces
// of the blocked one, the one kernel that writes into the fit, the border strip of a grown layout
size_t append_part_doubles(int npad);
int launch_append_small(bq_ctx *c, const double *V, int npad, int k, const double *z, long zstride,
                        double *part, const double *xn, const double *yn, int d,
                        const GaussParams &g, double tol, double *S, double *zn,
                        int *info);
int launch_append_rhs(bq_ctx *c, const double *yn, const double *vz, int k, double *X,
                      const double *S, int kp, double tol, int *info);
int launch_append_commit(bq_ctx *c, const AppendJob &a);
int launch_append_grow(bq_ctx *c, double *A, long lda, int r0, int ntot, int yrow,
                       const double *Aold, long ldold, int yold, int ncopy);
// shrinking a resident fit by k observations (remove.h): the pass into the new layout, the
// in-place form of a trailing removal, one block column of the update, the scalars
int launch_remove_compact(bq_ctx *c, const RemoveJob &r);
int launch_remove_trail(bq_ctx *c, double *A, long ldl, int yrow, double *pts, double *y, int d,
                        int n2, int n, int npad);
int launch_remove_step(bq_ctx *c, double *A, long lda, double *V, long ldv, int J, int nblocks,
                       double *Ms);
int launch_remove_finish(bq_ctx *c, const double *A, long lda, int yrow, int n, int npad,
                         double *dinv, double *out);

// ---- potrf.hip ------------------------------------------------------------------------
// scope of bq_ctx::sharing: how the chip is shared while the launches queued inside it run
struct Sharing {
    bq_ctx *c;
    int prev;
    Sharing(bq_ctx *c_, int how) : c(c_), prev(c_->sharing) { c->sharing = how; }
    ~Sharing() { c->sharing = prev; }
};
// scope of bq_ctx::cur: the launch helpers enqueue on `s` (the second stream of a look-ahead; the
// stream in force where a sweep forks only conditionally) until the scope ends, on every exit path
struct OnStream {
    bq_ctx *c;
    hipStream_t prev;
    OnStream(bq_ctx *c_, hipStream_t s) : c(c_), prev(c_->cur) { c->cur = s; }
    ~OnStream() { c->cur = prev; }
};
int auto_nb(const bq_ctx *c, int ntot, int batch);
// How the first ncols columns of `batch` matrices of ntot rows are eliminated, decided in ONE place
// (sweep_route): every enqueue asks again with the workspace on hand (a setter may have changed the
// answer since), every workspace is sized by the ws_doubles of the unlimited answer.
struct SweepRoute {
    // Slab: one launch per 64-column step (slab.h); Blocked: outer blocks of nb, look-ahead, the
    // slab tail of one or two matrices; Halves: two half-batches of it on the two streams;
    // DiagFirst: batches, diagonal block first (enqueue_potrf_dfirst)
    enum Kind { Slab, Blocked, Halves, DiagFirst } kind;
    int ntot, ncols, batch;
    int nb;                 // outer block (auto_nb)
    size_t ws_doubles;      // workspace the route uses (0: none)
    bool first_in_assembly; // Slab: an assembly launch can carry step 0 (FirstStep)
    int seed_cols;          // DiagFirst: columns to assemble before a seeded sweep (0: all)
    bool border_rows;       // a bordered system's results can come off its border rows
};
SweepRoute sweep_route(const bq_ctx *c, int ntot, int ncols, int batch,
                       size_t ws_on_hand = SIZE_MAX);
// what a caller tells the sweep besides its route
struct SweepArgs {
    bool first_done = false;     // the assembly carried step 0 (SweepRoute::first_in_assembly)
    bool skip_border = false;    // the results come off the border rows (SweepRoute::border_rows)
    SlabOut out{};               // Slab: the last step stores the read-out (scal != nullptr)
    GramSeed seed{};             // DiagFirst: only SweepRoute::seed_cols columns were assembled
    long long *stamps = nullptr; // Slab: bq_probe_c2_timeline's 160 stamps per step, for
    int stamped_steps = 0;       // this many steps
};
int enqueue_potrf_partial(bq_ctx *c, const SweepRoute &r, double *A, long lda, long astride,
                          double *dinv, int *info, double *ws, const SweepArgs &a = SweepArgs());
int enqueue_bordered(bq_ctx *c, const GramSeed &sys, int batch, double *A, long lda, long astride,
                     double *dinv, int *info, double *ws, size_t ws_len, double *scal, double *mean,
                     double *var, long mstride, bool rows, double work, long long *stamps = nullptr,
                     int stamped_steps = 0);

int enqueue_panel_solve(bq_ctx *c, double *A, long lda, long astride, int batch, int r0, int m2,
                        int K0, int KB, const double *rec, long rstride, bool one_launch);

// ---- sweeps.hip -----------------------------------------------------------------------
struct WideInv {
    const double *nr = nullptr; // -W^T of every block
    // the single-vector sweeps (trsv.h):
    const double *nt = nullptr; // -W (the transposes)
    const double *tt = nullptr; // T_J^T, T_J = W_J L[J, J-B] (blocks J >= B)
    const double *uu = nullptr; // U_J = L[J+B, J] W_J (all blocks but the last)
    const double *t = nullptr;  // T_J itself (rows of T contiguous: the fused row-sweep step)
    int B = 0;
};
inline int wide_block(int npad)
{
    // (round 5, profiles/r05_wide_b_check.txt, 256 against 512 on resident fits of 1024 / 1536 points:
    // posterior mean + variance at 256 points 0.064 -> 0.056 / 0.094 -> 0.073 ms, one-vector solve
    // 0.053 -> 0.039 / 0.070 -> 0.047 -- half the dependent steps --; the inverses cost 0.06 ms
    // more to rebuild after a refit: 0.43 -> 0.50 ms for refit + first posterior)
    return npad < 1024 ? std::min(npad, 256) : 512;
}
inline size_t wide_doubles(int npad) { return (size_t)npad * wide_block(npad); }
// NR, NT, TT, UU and the scratch of T before its transposition (a full B x B per block)
inline size_t wide_alloc_doubles(int npad)
{
    const size_t B = (size_t)wide_block(npad);
    return 5 * wide_doubles(npad) + B * B;
}
WideInv wide_views(const double *base, int npad);
// How a row sweep over a resident factor goes out, decided in ONE place each (sweeps.hip): the kind
// of the whole sweep (rows_route) and the form of a fused step's update (rows_update).  The sweeps
// ask these and report what they ran (bq_probe_sweep passes it on).
struct RowsRoute {
    // Step: one rows_step_kernel launch per block, split-k tiles (small systems, forward);
    // Fused: one launch per block, the update in LDS-staged or split-k tiles (rows_fused_kernel);
    // Gemm: two gemm_rows products per block (what neither takes, and every small backward sweep)
    enum Kind { Step, Fused, Gemm } kind;
    int B;        // columns per step (wide_block)
    int n_lds;    // Fused: steps whose update went out as 64 x 64 LDS-staged tiles ...
    int n_splitk; // ... and as 32 x 32 split-k tiles
};
enum class RowsUpdate { None, Lds, SplitK };
// tri: the triangular inverse (enqueue_inverse_rows: mrows = npad, forward)
RowsRoute rows_route(const bq_ctx *c, bool forward, int mrows, int npad, long ldl,
                     bool tri = false);
// the update of a fused step: mrows x nu entries, bp columns of the block solved one step earlier
RowsUpdate rows_update(bool forward, int mrows, int nu, int bp);
int compute_wide_inverses(bq_ctx *c, const double *L, long ldl, int npad, const double *dw,
                          double *nr);
// ws: trsv_flow_ws_doubles(npad, w.B) doubles for the one-launch form (nullptr: a launch per block)
int enqueue_forward_vec(bq_ctx *c, double *x, double *y, const double *L, long ldl, int npad,
                        WideInv w, double *ws = nullptr);
int enqueue_backward_vec(bq_ctx *c, double *x, double *y, const double *L, long ldl, int npad,
                         WideInv w, double *ws = nullptr);
int enqueue_forward_rows_blk(bq_ctx *c, double *X, long ldx, int mrows, const double *L, long ldl,
                             int npad, const double *dw);
// Y <- L^-T (npad x npad, ld npad); X: workspace of the same size.  Rows at or beyond a step's
// block are still unit vectors and sit out (N^3 / 3 flops); Y's strict lower triangle is not
// written (the caller clears it once)
int enqueue_inverse_rows(bq_ctx *c, double *X, double *Y, const double *L, long ldl, int npad,
                         WideInv w, RowsRoute *ran = nullptr);
// ran: the route the sweep took (rows_route, and the fused steps' update forms)
int enqueue_forward_rows(bq_ctx *c, double *Xin, double *Xout, long ldx, int mrows,
                         const double *L, long ldl, int npad, WideInv w, RowsRoute *ran = nullptr);
int enqueue_backward_rows(bq_ctx *c, double *Xin, double *Xout, long ldx, int mrows,
                          const double *L, long ldl, int npad, WideInv w, RowsRoute *ran = nullptr);
int solve_rows_host(bq_ctx *c, const double *L, long ldl, int n, int npad, WideInv w,
                    const double *B, int64_t nrhs, double *X);

// ---- moments.hip ----------------------------------------------------------------------
// The measure of an integral, as the caller's host arrays (include/bqhip.h has the three layouts):
//   GAUSS  N(a, b):                      a = mu, d;      b = Sigma, d x d column-major
//   BOX    uniform on prod_k [a_k, b_k]: a = lo, d;      b = hi, d
//   MIX    sum_c pi_c N(a_c, b_c):       a = mu, d x C;  b = C blocks Sigma_c;  pi: C weights
// This value is the only way a measure reaches launch_kernel_mean and the key of the KMEAN state.
struct Measure {
    enum Kind : int { GAUSS = 0, BOX = 1, MIX = 2 };
    Kind kind;
    int64_t C; // MIX: the components (as the caller gave them: checked by launch_kernel_mean)
    const double *pi, *a, *b;
    static Measure gauss(const double *mu, const double *cov)
    {
        return Measure{GAUSS, 1, nullptr, mu, cov};
    }
    static Measure box(const double *lo, const double *hi)
    {
        return Measure{BOX, 1, nullptr, lo, hi};
    }
    static Measure mix(int64_t C, const double *pi, const double *mu, const double *cov)
    {
        return Measure{MIX, C, pi, mu, cov};
    }
};
// a mixture's forms as the device reads them: C GaussForm<d> of diag(w^2) + Sigma_c about mu_c,
// then the C weights
inline size_t mix_form_doubles(int d, int C) { return (size_t)C * (d + d * d + 1) + C; }
// The kernel mean of the measure m under k = h^2 N(. | ., diag(w^2)): out[i] = kappa(x_i) at the n
// device points x, d x n, on the context's stream (n == 0: no launch), and, with kk, *kk = the
// prior variance of the integral, int int k m m, on the host.  GAUSS: int_K_kernel, kappa = h^2
// N(x | mu, diag(w^2) + cov), kk = h^2 N(0 | 0, diag(w^2) + 2 cov).  BOX: int_K_box_kernel.  MIX:
// int_K_mix_kernel over the forms in device memory at `forms` (mix_form_doubles; mix_forms below
// writes them), kk summed on the host over the GaussForm of diag(w^2) + Sigma_c + Sigma_c'.
// BQ_ERR_BAD_ARG, before anything is enqueued, for every illegal measure of include/bqhip.h: a
// NULL array, an entry that is not finite, lo_k >= hi_k, C out of range, a negative weight or
// weights that sum to zero, and a diag(w^2) + cov, or (with kk; GAUSS: always) a diag(w^2) + 2 cov
// or + Sigma_c + Sigma_c', whose host factor (GaussForm) fails.
int launch_kernel_mean(bq_ctx *c, int d, const double *x, int n, double h, const double *w,
                       const Measure &m, double *out, double *kk, const double *forms = nullptr);
// the forms of a legal mixture for int_K_mix_kernel, mix_form_doubles(d, m.C) doubles on the host
void mix_forms(int d, const double *w, const Measure &m, double *host);
// the transforms and constants of square-root-warped quadrature (types.h, SqForms) for the kernel
// (h, w) and the measure N(mu, cov), on the host.  BQ_ERR_BAD_ARG as launch_kernel_mean, and for a
// diag(w^2) + 2 S, S = (diag(w^-2) + cov^-1)^-1, whose host factor fails.
int sq_forms(bq_ctx *c, int d, double h, const double *w, const double *mu, const double *cov,
             SqForms *out);
// The marginal of a fit under a Gaussian or a box (marginal.h has the kernels and the one
// expression both kinds share; include/bqhip.h, bq_gp_marginal, the contract): everything the
// host works out of (h, w), the measure and the kept axes, as the kernels read it -- d x d
// matrices row-major with stride d, embedded at the axes' own indices.
struct MargPlan {
    int d = 0;
    bool box = false;
    unsigned keep = 0;           // bit k: axis k is kept
    double mu[BQ_MAXD] = {0};    // Gaussian: the measure's mean
    double lo[BQ_MAXD], hi[BQ_MAXD]; // the box's ends on the kept axes; -inf, +inf elsewhere
    double ls[BQ_MAXD * BQ_MAXD] = {0}; // inverse factor of Sigma_SS
    double bm[BQ_MAXD * BQ_MAXD] = {0}; // B = Sigma_IS Sigma_SS^-1
    double le[BQ_MAXD * BQ_MAXD] = {0}; // diag(1 / w_S), inverse factor of W_I + Sigma_c
    double g[BQ_MAXD * BQ_MAXD] = {0};  // the prior's transform of q - q'
    double lq = 0;                      // the constant of log pi_S
    double logc_e = 0, scale_e = 0;     // a cross entry's constant and factor
    double logc_p = 0, scale_p = 0, rvol = 1; // the prior's; 1 / vol_S of a box
    double h2 = 0;
    // box: int_K_box_kernel's form of kappa_box,I -- the ends on I, -inf and +inf on S, where
    // rl = 1 and the factor is exactly 1
    double ilo[BQ_MAXD], ihi[BQ_MAXD], rw[BQ_MAXD] = {0}, rl[BQ_MAXD] = {0};
};
// The plan of a call, or BQ_ERR_BAD_ARG before anything is allocated: the measure's own checks
// (launch_kernel_mean's, on all d axes), keep == NULL, a flag that is not 0 or 1, all flags set or
// none, a covariance that is not symmetric, and a Sigma_SS, W_I + Sigma_c or W_I + 2 Sigma_c whose
// host factor fails.  xq (d x M; NULL: not checked): a kept coordinate that is not finite.
int marginal_plan(bq_ctx *c, int d, double h, const double *w, const int32_t *keep,
                  const Measure &m, const double *xq, int64_t M, MargPlan *out);
// colv[j] = kappa_box,I(x_j), h^2 included, at the n device points x (a box's plan only)
int launch_marginal_colv(bq_ctx *c, const MargPlan &pl, const double *x, int n, double *colv);
// K (Mp x npad, ld ldk) = c(xq, x) with its zero padding (marginal_cross_kernel)
int launch_marginal_cross(bq_ctx *c, const MargPlan &pl, const double *xq, int M, int Mp,
                          const double *x, int n, int npad, const double *colv, double *K, long ldk);
// mean = c(xq, x) alpha without a matrix (marginal_mean_kernel)
int launch_marginal_mean(bq_ctx *c, const MargPlan &pl, const double *xq, int M, const double *x,
                         int n, const double *colv, const double *alpha, double *mean);
// P (Mp x Mp, ld ldp; NULL: none) and / or its diagonal (diag; accum: added to what is there)
int launch_marginal_prior(bq_ctx *c, const MargPlan &pl, const double *xq, int M, int Mp, double *P,
                          long ldp, double *diag, int accum);

// ---- linalg.hip -----------------------------------------------------------------------
// factor one ntot x ntot device matrix on the context's panel scratch (dinv: BQ_DINV_STRIDE)
int potrf_one(bq_ctx *c, double *A, long lda, int ntot, double *dinv, int *info);
// that scratch grown to what potrf_one of an ntot x ntot matrix uses (a caller that allocates
// everything before it enqueues anything)
int grow_panel_ws(bq_ctx *c, int ntot);

} // namespace bqh

// ---- handle types (plan.hip, fit.hip) ---------------------------------------------------
struct bq_plan {
    int nprob = 0, d = 0, n = 0, M = 0;
    Layout L{};
    long lda = 0, astride = 0;
    DevBuf A, pts, y, gp, dinv, info, scal, mean, var;
    DevBuf panel; // scratch panel columns of the one-launch slab sweep (small systems)
    std::vector<GaussParams> hgp;
    bool has_inputs = false;
    // the launch sequence of a plan is static: it is captured once into a hipGraph
    // and replayed (cuts the host launch cost of the ~50 short kernels of a step)
    CapturedSeq seq;
    double *hres = nullptr; // pinned staging of bq_plan_results: [scal 4 nb | info nb | mean | var]
    double *hin = nullptr;  // pinned staging of a small plan's inputs (bq_plan_set_inputs)
    size_t hin_len = 0;
    bool in_flight = false; // the scatter out of hin may not have run yet
    ~bq_plan()
    {
        if (hres)
            (void)hipHostFree(hres);
        if (hin)
            (void)hipHostFree(hin);
    }
};

// The layout of a fit's system and the seven buffers sized by it: allocated together, all or none,
// and swapped together when a fit moves to another layout (fit_adopt).
struct FitCore {
    int npad = 0;
    long ldl = 0;
    Layout L{}; // layout of the fit system (M = 0, y row)
    DevBuf A;     // ntot x ntot bordered factor: L in [0,npad)^2, z in row yrow
    DevBuf pts;   // d x ntot
    DevBuf y;     // npad
    DevBuf dinv;  // npad reciprocal diagonal (+ BQ_DINV_STRIDE scratch for the factorisation)
    DevBuf panel; // scratch panel columns of the one-launch slab sweep
    DevBuf dw;    // diag_winv_kernel records of the resident factor (MFMA solves in the sweeps)
    DevBuf alpha; // npad
    // The layout of n points in d dimensions and its buffers.  A failure leaves nothing allocated,
    // no layout, and the caller's words (printf-style) as the error: "<what>: <the HIP error>"
    __attribute__((format(printf, 5, 6))) int alloc(bq_ctx *c, int d, int n, const char *what, ...)
    {
        L = bqh::make_layout(n, 0, true);
        npad = L.npad;
        ldl = bqh::pick_ld(L.ntot);
        const size_t np = (size_t)npad, nt = (size_t)L.ntot;
        hipError_t e = hipSuccess;
        auto get = [&](DevBuf &b, size_t doubles) {
            if (e == hipSuccess)
                e = b.alloc(sizeof(double) * doubles);
        };
        get(A, (size_t)ldl * nt), get(pts, (size_t)d * nt), get(y, np);
        get(dinv, np + BQ_DINV_STRIDE);
        get(panel, bqh::sweep_route(c, L.ntot, L.ntot, 1).ws_doubles);
        get(dw, BQ_DINV_HALF * (np / 64)), get(alpha, np);
        if (e == hipSuccess)
            return BQ_OK;
        (void)hipGetLastError();
        FitCore none;
        swap(none); // (what was allocated goes with it)
        char msg[160];
        va_list ap;
        va_start(ap, what);
        vsnprintf(msg, sizeof msg, what, ap);
        va_end(ap);
        return bqh::fail(c, e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP, "%s: %s", msg,
                         hipGetErrorString(e));
    }
    void swap(FitCore &o)
    {
        std::swap(npad, o.npad), std::swap(ldl, o.ldl), std::swap(L, o.L);
        A.swap(o.A), pts.swap(o.pts), y.swap(o.y), dinv.swap(o.dinv);
        panel.swap(o.panel), dw.swap(o.dw), alpha.swap(o.alpha);
    }
};

struct bq_fit : FitCore {
    int d = 0, n = 0;
    double h = 0, s = 0, w[BQ_MAXD] = {0};
    GaussParams g{};
    DevBuf gp;    // GaussParams
    DevBuf misc;  // info (int) + scal[4], then 2 x 64 doubles: the posterior of the border points
                  // of bq_gp_refit_predict (one read-back for all of it)
    // ---- derived state: what the handle holds beyond the factor, z and the scalars -------------
    // One bit of `have` per result, set by the one function that computes it and cleared by the
    // two events below.  This table is the only statement of either (DESIGN 4e repeats it):
    //   bit       what is there                                     from        set by
    //   DW        dw: 16 x 16 inverses of the factor's diagonal     the factor  fit_dw
    //   WIDE      wide: -W^T of the B-wide diagonal blocks          DW          fit_wide
    //   ZC        wz: z = L^-1 y contiguous (the factor's y row     z           fit_zc
    //             has stride ldl: the row reductions then read
    //             one line per 8 entries, not one per entry)
    //   ALPHA     alpha = L^-T z                                    WIDE, z     fit_alpha
    //   Y         gY: Y = L^-T, zero below its diagonal (gX: the    WIDE        fit_y
    //             sweep's workspace)
    //   PROD      gX, hB: the Hessian's products stage (Kxx^-1,     Y, ALPHA    fit_prod
    //             the d products, the vectors D_p a and
    //             Kxx^-1 D_p a), which the Hessian's sums and
    //             both cross-validation gradients read
    //   HESS      hess                                              PROD        bq_gp_logml_hess
    //   LOO       loo: mu | var | lp; loo_total                     Y, ALPHA    fit_loo
    //   LOO_GRAD  loo_grad                                          PROD, LOO   bq_gp_loo_grad
    //   DKZ       dkz: u = Kxx^-1 alpha and z_k = Kxx^-1 (D_k       ALPHA, WIDE fit_dkz
    //             alpha) as the rows of a 64 x npad matrix (its
    //             second half: the row sweeps' workspace)
    //   TREND     trend: G = L^-1 H as rows, the factor of          WIDE, z,    fit_trend
    //             A = G^T G, A^-1, beta, alpha_t and the scalars    the key
    //             of the polynomial trend with the key (degree,
    //             c, rho) in tr_key; a call with another key
    //             recomputes it
    //   KMEAN     kmean: kappa_X = the kernel mean of the measure   WIDE,       fit_kmean
    //             (a Gaussian, a box or a mixture of Gaussians)     the key
    //             at the fit's points, b = L^-1 kappa_X, b.b, and
    //             a mixture's forms; km_kk = the prior variance of
    //             the integral, with the key (the measure's kind
    //             and numbers) in km_key; a call with another key
    //             recomputes it.  Nothing of it depends on the
    //             targets: bq_gp_integral's mean is one dot product
    //             b.z with the current z
    //   SQW       sqw: square-root-warped quadrature under the      WIDE, ALPHA, fit_sqw
    //             measure N(mu, Sigma): r = W(X, X) alpha, b_w =    the key
    //             L^-1 r, the fit's transformed points with alpha,
    //             and on the host b_w.b_w, qq = alpha^T Q alpha and
    //             sq = alpha.r, with the key (mu, Sigma) in sq_key;
    //             a call with another key recomputes it.  All of
    //             it depends on the targets
    // (z is the targets through the factor.)  A bit is never set while a bit it is computed from is
    // clear: every producer runs the producers of what it reads first, and both events clear a bit
    // together with everything computed from it.
    enum : unsigned {
        DW = 1u << 0,
        WIDE = 1u << 1,
        ZC = 1u << 2,
        ALPHA = 1u << 3,
        Y = 1u << 4,
        PROD = 1u << 5,
        HESS = 1u << 6,
        LOO = 1u << 7,
        LOO_GRAD = 1u << 8,
        DKZ = 1u << 9,
        TREND = 1u << 10,
        KMEAN = 1u << 11,
        SQW = 1u << 12,
        // the events: a (re)factorisation, an append, a removal ...
        FACTOR_CHANGED =
            DW | WIDE | ZC | ALPHA | Y | PROD | HESS | LOO | LOO_GRAD | DKZ | TREND | KMEAN | SQW,
        // ... and bq_gp_set_y (the factor's own inverses stay, and so does KMEAN)
        TARGETS_CHANGED = ZC | ALPHA | Y | PROD | HESS | LOO | LOO_GRAD | DKZ | TREND | SQW,
    };
    unsigned have = 0;
    void drop(unsigned event) { have &= ~event; }
    DevBuf wide;                  // wide_alloc_doubles(npad), allocated on the first sweep
    DevBuf wV, wV2, wx, wout, wz; // prediction workspaces, grown on demand and kept
    // posterior samples (bq_gp_sample): GaussParams without s^2 | info | Sigma | the matrix being
    // factored (a ladder of more than one entry) | Z | out, grown on demand and kept
    DevBuf smp;
    // pivoted partial Cholesky of a posterior (bq_gp_pivchol): the device state | gain | piv | d |
    // the taken rows | the workgroups' candidates | the slices' partial sums (PivcholPlan), grown
    // on demand and kept; the factor's columns follow V in wV2
    DevBuf pvc;
    // designs that minimise the integrated variance (bq_gp_ivr): the steps' workspace (IvrPlan)
    // and T = Sigma(xc, xr), Ap x Rp, grown on demand and kept; the c columns follow V in wV2
    DevBuf ivr, ivrT;
    // the integral of the fit under a measure (bq_gp_integral, bq_gp_zdesign and their _box and
    // _mix twins): kappa_X (npad) | b (npad) | b.b, b.z, allocated on the first call and kept; a
    // mixture's forms on the device (kmform, mix_form_doubles of the largest mixture) and on their
    // way there (km_hform: read by a copy on the stream, so it lives as long as the fit),
    // allocated on the first call with a mixture; the measure the state was computed for --
    // [kind | mu d | Sigma d x d], [kind | lo d | hi d] or [kind, C | pi C | mu d x C | Sigma
    // d x d x C], zeros behind, compared byte by byte -- and the host's share of the state
    DevBuf kmean, kmform;
    std::vector<double> km_hform;
    static constexpr size_t KM_KEY_LEN =
        2 + (size_t)BQ_MEASURE_MAX_COMP * (1 + BQ_MAXD + BQ_MAXD * BQ_MAXD);
    double km_key[KM_KEY_LEN] = {0};
    double km_kk = 0, km_bb = 0;
    // designs that lower the integral's variance (bq_gp_zdesign): the steps' workspace (ZdPlan),
    // grown on demand and kept; the c columns follow V in wV2
    DevBuf zd;
    // square-root-warped quadrature (bq_gp_sqintegral, bq_gp_sqdesign): the state r (npad) | b_w
    // (npad) | b_w.b_w, qq, sq (32) | the fit's 2 d coordinates (npad x 2 d) | their weights alpha
    // (npad), then scratch: the d coordinates of Q | their weights | Q's row sums | the pair sums'
    // slices -- allocated on the first call and kept; the measure it was computed for and the
    // host's share of the state; the candidates' coordinates and slices of a design, grown on
    // demand and kept
    DevBuf sqw, sqc;
    double sq_key[BQ_MAXD + BQ_MAXD * BQ_MAXD] = {0};
    double sq_bb = 0, sq_qq = 0, sq_sq = 0;
    // the log-ML gradient (bq_gp_logml_grad): Y and the sweep's partial sums (npad x npad each),
    // allocated on the first gradient; the product's partials and the d + 2 results
    DevBuf gY, gX, gpart;
    // the log-ML Hessian (bq_gp_logml_hess): Kxx^-1 takes gX once the sweep is done with it; the d
    // products Kxx^-1 dK/dw_k, the vectors and the partial sums (hess_ws_doubles) in hB, allocated
    // on the first Hessian
    DevBuf hB;
    double hess[(BQ_MAXD + 2) * (BQ_MAXD + 2)] = {0};
    // leave-one-out (bq_gp_loo, bq_gp_loo_grad): diag Kxx^-1, the row sums, mean / variance / log
    // density per point and the partial sums (loo_ws_doubles), allocated on the first call
    DevBuf loo;
    double loo_total = 0, loo_grad[BQ_MAXD + 2] = {0};
    // leave-group-out (bq_gp_lgo, bq_gp_lgo_grad): the groups, their blocks and partial sums
    // (lgo_ws_doubles), grown on demand and kept.  Nothing of it is a result that `have` tracks:
    // every call computes its own groups anew.
    DevBuf lgo;
    // the posterior's derivatives in the hyper-parameters (bq_gp_predict_dtheta): [u, z_1 .. z_d]
    // as rows, 64 x npad, and as much again for the two row sweeps that solve them (fit_dkz),
    // allocated on the first call; the quad product's partial sums, grown on demand and kept
    DevBuf dkz, wq;
    // the polynomial trend (bq_gp_trend, bq_gp_predict_trend): the state (TrendPlan), allocated on
    // the first call and kept, and the basis it was computed for; the basis rows of a prediction's
    // points (Mp x 64), grown on demand and kept; the route the last prediction took
    // (bq_gp_trend_last_route)
    DevBuf trend, wphi;
    TrendBasis tr_key{};
    int tr_route = -1, tr_gemm = -1;
    // the single-vector sweeps (trsv.h): x | y, 2 npad doubles, and their captured launch
    // chains -- [0] solve (forward + backward), [1] backward into alpha, [2] forward; the
    // pointers survive a refit, so the graphs do too
    DevBuf vec;
    double *hvec = nullptr; // pinned staging of one vector in / out (npad doubles): a copy from
                            // pageable memory is staged and synchronised by the runtime, which
                            // was half of a single-vector solve's wall time at N = 4096
    double *hio = nullptr;  // pinned staging of a prediction's points in and mean / variance
                            // (bq_gp_predict_grad: and the gradients) out
    size_t hio_len = 0;
    double *hfit = nullptr; // pinned staging of a (re)fit: [results 8 + 128 | GaussParams | 63 d
                            // border points] -- the hyper-parameter loop's body is three small copies
    CapturedSeq vseq[3];
    ~bq_fit()
    {
        if (hvec)
            (void)hipHostFree(hvec);
        if (hio)
            (void)hipHostFree(hio);
        if (hfit)
            (void)hipHostFree(hfit);
    } // (the captured sweeps go with vseq)
    // false from the start of a (re)factorisation until it has succeeded: a refit that hits a
    // non-positive pivot leaves L, dinv, dw and the scalars overwritten with garbage
    bool valid = false;
    // true after bq_gp_set_y until the next (re)fit: the targets changed, the factor did not
    bool stale = false;
    double logml = 0, logdet = 0, qf = 0;
};

namespace bqh {
// An on-demand buffer of a fit: buf holds at least `bytes` (kept between calls), or the call fails
// with "<what> (<bytes> bytes): <the HIP error>" and buf is left empty
inline int fit_grow(bq_ctx *c, DevBuf &buf, size_t bytes, const char *what)
{
    if (buf.bytes >= bytes)
        return BQ_OK;
    const hipError_t e = buf.alloc(bytes);
    if (e == hipSuccess)
        return BQ_OK;
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP, "%s (%zu bytes): %s", what,
                bytes, hipGetErrorString(e));
}

// A fit takes over the core of another layout (a growing append, a removal that is not in place;
// the stream is idle).  Every workspace sized by the old padding goes, and so do the captured
// sweeps, which hold the old pointers; the old core leaves in `core`, for the caller to free.
inline void fit_adopt(bq_fit *f, FitCore &core)
{
    f->swap(core);
    for (DevBuf *b : {&f->wide, &f->vec, &f->wV, &f->wV2, &f->wz, &f->gY, &f->gX, &f->gpart, &f->hB,
                      &f->loo, &f->lgo, &f->dkz, &f->wq, &f->trend, &f->kmean, &f->sqw})
        b->release();
    if (f->hvec)
        (void)hipHostFree(f->hvec);
    f->hvec = nullptr;
    for (CapturedSeq &v : f->vseq)
        v.drop();
}
} // namespace bqh

namespace bqh {
// fit.hip: shared with moments.hip
int check_fit(bq_ctx *c, const bq_fit *f);
int fit_dw(bq_ctx *c, bq_fit *f);
int fit_wide(bq_ctx *c, bq_fit *f, WideInv &w);
int fit_vec(bq_ctx *c, bq_fit *f);
int fit_alpha(bq_ctx *c, bq_fit *f);
int fit_dkz(bq_ctx *c, bq_fit *f);
int fit_zc(bq_ctx *c, bq_fit *f);
// Replays a chain of sweep launches over a fit's own buffers from the slot's captured hipGraph (a
// sweep is 2 npad / B launches of 2-8 us each: enqueued one by one the host is the bottleneck).
template <class F>
int fit_replay(bq_ctx *c, bq_fit *f, int slot, F &&enqueue)
{
    // (a one-launch sweep is two memsets and a kernel: enqueued directly it costs the host less
    // than a graph launch does)
    if (trsv_flow_ok(c, f->npad, wide_block(f->npad)))
        return enqueue();
    return f->vseq[slot].run(c, enqueue);
}
// A one-launch sweep whose hand-off timed out (trsvflow.h: a shared device, a lost slot) has raised
// the context's abort word and every spinner has left: the results of `attempt` are garbage.
// Degrade, do not fail: clear the word, count the event (bq_ctx_stats) and re-issue the SAME
// solve -- `attempt` restages its inputs and ends with the stream synchronised -- on the per-block
// kernels, which compute the same bits (test_flow_sweeps_same_bits_as_per_block_launches).
bool flow_timed_out(bq_ctx *c);
template <class F>
int with_flow_fallback(bq_ctx *c, F &&attempt)
{
    int st = attempt();
    if (st != BQ_OK || !flow_timed_out(c))
        return st;
    ++c->n_flow_fallback;
    const int saved = c->cfg.trsv_flow;
    c->cfg.trsv_flow = 0;
    st = attempt();
    c->cfg.trsv_flow = saved;
    // the retry must not have gone through a one-launch sweep again (a captured graph that still
    // holds one: a slot captured under another trsv_flow is dropped, CapturedSeq) -- if the word
    // is up again the results are garbage and the call says so
    if (st == BQ_OK && flow_timed_out(c))
        return fail(c, BQ_ERR_HIP, "a sweep's hand-off timed out again on the per-block kernels");
    return st;
}
// plan.hip: new kernel parameters for every problem of a plan, nothing else re-uploaded
int plan_set_params(bq_ctx *c, bq_plan *p, const double *h, const double *w, const double *s);
// plan.hip: the launch sequence of one pass of a plan (probe.hip, bq_probe_c2_timeline, runs it
// eagerly with its stamps)
int plan_enqueue(bq_ctx *c, bq_plan *p, long long *stamps = nullptr, int stamped_steps = 0);
} // namespace bqh
