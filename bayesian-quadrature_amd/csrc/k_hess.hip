// k_hess.hip -- the log-ML Hessian's kernels (hess.h), the leave-one-out kernels that read its
// products (loo.h) and their leave-group-out counterparts (lgo.h), the posterior's derivatives in
// the hyper-parameters, which generate the same derivative operand (ptheta.h), and their launchers.
#include "host.h"
#include "hess.h"
#include "loo.h"
#include "lgo.h"
#include "ptheta.h"

namespace bqh {

// device workspace of one Hessian beside Ki: [B_1 .. B_d | V | Z | partials | sums]
static size_t hess_tiles(int npad) { return (size_t)(npad / 64) * (size_t)(npad / 64); }
static size_t hess_off_v(int npad, int d) { return (size_t)d * npad * npad; }
static size_t hess_off_part(int npad, int d) { return hess_off_v(npad, d) + 2 * (size_t)(d + 2) * npad; }
static size_t hess_off_sums(int npad, int d)
{
    return hess_off_part(npad, d) + hess_tiles(npad) * (size_t)std::max(hess_ng(d), hess_nt(d));
}
size_t hess_ws_doubles(int npad, int d)
{
    return hess_off_sums(npad, d) + (size_t)(hess_ng(d) + hess_nt(d) + hess_nq(d));
}
// its views; T = const double for the stages that only read it (loo_grad_run, launch_lgo_grad)
template <class T>
struct HessWs { T *B, *V, *Z, *part, *sums; };
template <class T>
static HessWs<T> hess_views(T *ws, int npad, int d)
{
    T *V = ws + hess_off_v(npad, d);
    return {ws, V, V + (size_t)(d + 2) * npad, ws + hess_off_part(npad, d), ws + hess_off_sums(npad, d)};
}

// what every launcher of this unit asks of d and npad, and the message of those that ask no more
static bool bad_d_npad(int d, int npad) { return d < 1 || d > BQ_MAXD || (npad % 64); }
static int fail_d_npad(bq_ctx *c, const char *what)
{
    return fail(c, BQ_ERR_BAD_ARG, "%s: d in [1, %d], npad a multiple of 64", what, BQ_MAXD);
}

// out[c] = the sum over i < nitem of part[i item_stride + c c_stride], c < nc, a workgroup per c
// (host.h: k_reduce.hip folds the trend's sums with it)
void launch_fold(bq_ctx *c, const double *part, int nitem, long item_stride, long c_stride,
                        int nc, double *out)
{
    hipLaunchKernelGGL(fold_kernel<FoldPlain>, dim3((unsigned)nc), dim3(256), 0, c->stream, part, nitem,
                       item_stride, c_stride, nc, FoldPlain{}, out);
}

// Workgroup tile of the products: the tall 256 x 64 tile where the gradient's product takes its
// 128 x 128 tile (as many workgroups), else 64 x 64
static bool hess_tall(const bq_ctx *c, int npad) { return grad_tile(c, npad) == 128; }

template <int D>
static void hess_launch_prod(bq_ctx *c, bool tall, double *C, const double *A, const double *Q,
                             const HessJob &hj, int kdim)
{
    const unsigned gy = (unsigned)hj.npad / 64;
    if (tall)
        hipLaunchKernelGGL((hess_prod_kernel<D, 4, 1, 4, 4>), dim3((unsigned)(hj.npad + 255) / 256, gy),
                           dim3(256), 0, c->stream, C, A, Q, hj, kdim);
    else
        hipLaunchKernelGGL((hess_prod_kernel<D, 2, 2, 2, 2>), dim3(gy, gy), dim3(256), 0, c->stream,
                           C, A, Q, hj, kdim);
}

// The products stage: Ki = Y Y^T, the d products B_k = Ki D_k, V = D_p a and Z = Ki V
template <int D>
static int hess_run_products(bq_ctx *c, const double *Y, double *Ki, double *ws, const HessJob &hj,
                             const double *y, double h, double s)
{
    const int npad = hj.npad;
    const bool tall = hess_tall(c, npad);
    const HessWs<double> w = hess_views(ws, npad, D);
    const double n3 = (double)npad * npad * npad;
    {
        Bracket br(c, BQ_K_GEMM, n3 * 2.0 / 3.0);
        hess_launch_prod<0>(c, tall, Ki, Y, Y, hj, 0);
        HIPCHK(c, hipGetLastError());
    }
    for (int k = 0; k < D; ++k) {
        Bracket br(c, BQ_K_GEMM, 2.0 * n3);
        hess_launch_prod<D>(c, tall, w.B + (size_t)k * npad * npad, Ki, nullptr, hj, k);
        HIPCHK(c, hipGetLastError());
    }
    Bracket br(c, BQ_K_REDUCE);
    hipLaunchKernelGGL(hess_dka_kernel<D>, dim3((unsigned)npad / 16), dim3(256), 0, c->stream, hj, y,
                       2.0 / h, 2.0 * s, w.V);
    hipLaunchKernelGGL(hess_kiv_kernel, dim3((unsigned)npad / 4), dim3(256), 0, c->stream, Ki, hj.n,
                       npad, D + 2, w.V, w.Z);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// The sums stage, over what the products stage left in Ki and ws
template <int D>
static int hess_run_sums(bq_ctx *c, const double *Ki, double *ws, const HessJob &hj)
{
    const int npad = hj.npad, n = hj.n;
    const HessWs<double> w = hess_views(ws, npad, D);
    Bracket br(c, BQ_K_REDUCE);
    const unsigned g64 = (unsigned)npad / 64;
    const int nwg = (int)(g64 * g64);
    // (a tile's partial of sum c at part[c nwg + tile])
    hipLaunchKernelGGL(hess_gsum_kernel<D>, dim3(g64, g64), dim3(256), 0, c->stream, Ki, hj, w.part);
    launch_fold(c, w.part, nwg, 1, nwg, hess_ng(D), w.sums);
    hipLaunchKernelGGL(hess_trace_kernel<D>, dim3(g64, g64), dim3(256), 0, c->stream, Ki, w.B, hj,
                       w.part);
    launch_fold(c, w.part, nwg, 1, nwg, hess_nt(D), w.sums + hess_ng(D));
    hipLaunchKernelGGL(hess_quad_kernel, dim3(1), dim3(256), 0, c->stream, w.V, w.Z, n, npad, D + 2,
                       w.sums + hess_ng(D) + hess_nt(D));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// The Hessian's products stage: Ki = Y Y^T, B_k = Ki D_k, V = D_p a, Z = Ki V from Y = L^-T (npad x
// npad, zero below its diagonal) and the fit's alpha.  Ki: npad^2 doubles, left holding Kxx^-1; ws:
// hess_ws_doubles(npad, d).
int launch_hess_products(bq_ctx *c, int d, const double *Y, double *Ki, double *ws,
                         const HessJob &hj, const double *y, double h, double s)
{
    if (bad_d_npad(d, hj.npad))
        return fail_d_npad(c, "hess_products");
    int st = BQ_OK;
    BQ_DISPATCH_D(d, st = hess_run_products<D>(c, Y, Ki, ws, hj, y, h, s));
    return st;
}

// The sums of one Hessian (types.h: hess_ng + hess_nt + hess_nq of them, at *sums inside ws) from
// what launch_hess_products left in Ki and ws since the fit last changed.
int launch_hess_sums(bq_ctx *c, int d, const double *Ki, double *ws, const HessJob &hj,
                     const double **sums)
{
    if (bad_d_npad(d, hj.npad))
        return fail_d_npad(c, "hess_sums");
    int st = BQ_OK;
    *sums = hess_views(ws, hj.npad, d).sums;
    BQ_DISPATCH_D(d, st = hess_run_sums<D>(c, Ki, ws, hj));
    return st;
}

// ---- leave-one-out (loo.h) ---------------------------------------------------------------
// device workspace of one fit's LOO: [k | q | t_1 .. t_d | mu | var | lp | partials | total, grad]
static int loo_chunks(int npad) { return (npad + BQ_LOO_CW - 1) / BQ_LOO_CW; }
static size_t loo_off_part(int npad, int d) { return (size_t)(d + 5) * npad; }
static size_t loo_off_out(int npad, int d)
{
    return loo_off_part(npad, d) + (size_t)(1 + d) * loo_chunks(npad) * npad;
}
size_t loo_ws_doubles(int npad, int d) { return loo_off_out(npad, d) + (size_t)(d + 3); }

// mu, var, lp (n each, at *vecs, npad apart) and L_loo (at *total) from Y = L^-T, alpha and y
int launch_loo(bq_ctx *c, int d, const double *Y, const double *alpha, const double *y, int n,
               int npad, double *ws, const double **vecs, const double **total)
{
    if (bad_d_npad(d, npad))
        return fail_d_npad(c, "loo");
    double *kd = ws, *mu = ws + (size_t)(d + 2) * npad;
    double *part = ws + loo_off_part(npad, d), *out = ws + loo_off_out(npad, d);
    const int nch = loo_chunks(npad);
    Bracket br(c, BQ_K_REDUCE);
    hipLaunchKernelGGL(loo_diag_kernel, dim3((unsigned)npad / 64, (unsigned)nch), dim3(256), 0,
                       c->stream, Y, n, npad, part);
    hipLaunchKernelGGL(loo_fold_kernel, dim3((unsigned)(npad + 255) / 256, 1), dim3(256), 0,
                       c->stream, part, nch, npad, kd);
    hipLaunchKernelGGL(loo_point_kernel, dim3(1), dim3(256), 0, c->stream, y, alpha, kd, n, mu,
                       mu + npad, mu + 2 * (size_t)npad, out);
    HIPCHK(c, hipGetLastError());
    *vecs = mu;
    *total = out;
    return BQ_OK;
}

template <int D>
static int loo_grad_run(bq_ctx *c, const double *Ki, const double *hws, const double *alpha, int n,
                        int npad, double h, double s, double s2, double *ws)
{
    const HessWs<const double> hw = hess_views(hws, npad, D);
    double *kd = ws, *q = ws + npad;
    double *part = ws + loo_off_part(npad, D), *out = ws + loo_off_out(npad, D);
    const int nch = loo_chunks(npad);
    Bracket br(c, BQ_K_REDUCE);
    hipLaunchKernelGGL(loo_rows_kernel<D>, dim3((unsigned)npad / 64, (unsigned)nch), dim3(256), 0,
                       c->stream, Ki, hw.B, n, npad, part);
    hipLaunchKernelGGL(loo_fold_kernel, dim3((unsigned)(npad + 255) / 256, 1 + D), dim3(256), 0,
                       c->stream, part, nch, npad, q);
    hipLaunchKernelGGL(loo_grad_kernel<D>, dim3(1), dim3(256), 0, c->stream, alpha, kd, q,
                       q + npad, hw.Z, n, npad, 2.0 / h, s, s2, out + 1);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// The d + 2 entries of dL_loo / dtheta (at *grad) from what launch_loo left in ws (k) and the
// Hessian's products stage left in Ki and hws (B_k, Z).
int launch_loo_grad(bq_ctx *c, int d, const double *Ki, const double *hws, const double *alpha,
                    int n, int npad, double h, double s, double s2, double *ws, const double **grad)
{
    if (bad_d_npad(d, npad))
        return fail_d_npad(c, "loo_grad");
    int st = BQ_OK;
    *grad = ws + loo_off_out(npad, d) + 1;
    BQ_DISPATCH_D(d, st = loo_grad_run<D>(c, Ki, hws, alpha, n, npad, h, s, s2, ws));
    return st;
}

// ---- leave-group-out (lgo.h) ------------------------------------------------------------
static_assert(BQ_LGO_MAXB == BQ_LGO_MAX, "lgo.h's blocks hold the ABI's largest group");
// Columns per workgroup of the block products: at most 8 chunks (their partials are T x 64
// doubles per chunk and product), and no chunk below 256 columns
static int lgo_cw(int npad) { return (std::max(256, npad / 8) + BQ_LGO_SLAB - 1) / BQ_LGO_SLAB * BQ_LGO_SLAB; }
static int lgo_chunks(int npad) { return (npad + lgo_cw(npad) - 1) / lgo_cw(npad); }
// idx (T) | start (G + 1) | flag | bundle (up to G + 1), in doubles
static size_t lgo_ints(long T, long G) { return ((size_t)T + 2 * (size_t)G + 3 + 1) / 2; }
static size_t lgo_off_part(int d, long T, long G)
{
    return lgo_ints(T, G) + (size_t)T * (64 + 3) + (size_t)G * (2 + d + 2) + (size_t)(d + 3);
}
static size_t lgo_part_doubles(int npad, long T) { return (size_t)lgo_chunks(npad) * T * 64; }
size_t lgo_ws_doubles(int npad, int d, long T, long G, bool grad)
{
    return lgo_off_part(d, T, G) + (size_t)(grad ? 2 + d : 1) * lgo_part_doubles(npad, T);
}
LgoWs lgo_views(double *ws, int npad, int d, long T, long G)
{
    LgoWs w;
    w.idx = reinterpret_cast<int *>(ws);
    w.start = w.idx + T;
    w.flag = w.start + G + 1;
    w.bundle = w.flag + 1;
    w.sig = ws + lgo_ints(T, G);
    w.r = w.sig + (size_t)T * 64;
    w.mu = w.r + T;
    w.var = w.mu + T;
    w.lp = w.var + T;
    w.ar = w.lp + G;
    w.gpart = w.ar + G;
    w.out = w.gpart + (size_t)G * (d + 2);
    w.part = ws + lgo_off_part(d, T, G);
    return w;
}

template <int MODE>
static void lgo_launch_blocks(bq_ctx *c, int maxb, unsigned nprod, const double *A, const double *P,
                              int n, int npad, long T, long NB, const LgoWs &w, double *part)
{
    const dim3 grid((unsigned)NB, (unsigned)lgo_chunks(npad), nprod);
    const int cw = lgo_cw(npad);
    if (maxb <= 16)
        hipLaunchKernelGGL((lgo_block_kernel<MODE, 1>), grid, dim3(256), 0, c->stream, A, P, n, npad,
                           cw, w.idx, w.start, w.bundle, T, part);
    else if (maxb <= 32)
        hipLaunchKernelGGL((lgo_block_kernel<MODE, 2>), grid, dim3(256), 0, c->stream, A, P, n, npad,
                           cw, w.idx, w.start, w.bundle, T, part);
    else
        hipLaunchKernelGGL((lgo_block_kernel<MODE, 4>), grid, dim3(256), 0, c->stream, A, P, n, npad,
                           cw, w.idx, w.start, w.bundle, T, part);
}

int launch_lgo(bq_ctx *c, const double *Y, const double *alpha, const double *y, int n, int npad,
               int d, long T, long G, long NB, int maxb, const LgoWs &w)
{
    if (bad_d_npad(d, npad) || maxb < 1 || maxb > BQ_LGO_MAXB || G < 1 || T < G ||
        NB < 1 || NB > G)
        return fail(c, BQ_ERR_BAD_ARG, "lgo: d in [1, %d], npad a multiple of 64, groups of 1 .. %d",
                    BQ_MAXD, BQ_LGO_MAXB);
    Bracket br(c, BQ_K_REDUCE);
    lgo_launch_blocks<LGO_YY>(c, maxb, 1, Y, nullptr, n, npad, T, NB, w, w.part);
    hipLaunchKernelGGL(lgo_group_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, w.part,
                       lgo_chunks(npad), T, w.idx, w.start, alpha, y, w.sig, w.r, w.mu, w.var, w.lp,
                       w.ar, w.flag);
    launch_fold(c, w.lp, (int)G, 1, 1, 1, w.out);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_lgo_grad(bq_ctx *c, int d, const double *Ki, const double *hws, int n, int npad, long T,
                    long G, long NB, int maxb, double h, double s, double s2, const LgoWs &w)
{
    if (bad_d_npad(d, npad) || maxb < 1 || maxb > BQ_LGO_MAXB || G < 1 || T < G ||
        NB < 1 || NB > G)
        return fail(c, BQ_ERR_BAD_ARG, "lgo_grad: d in [1, %d], npad a multiple of 64, groups of 1 .. %d",
                    BQ_MAXD, BQ_LGO_MAXB);
    const HessWs<const double> hw = hess_views(hws, npad, d);
    double *gp = w.part + lgo_part_doubles(npad, T); // [1 + d][nchunk][T][64]
    Bracket br(c, BQ_K_REDUCE);
    lgo_launch_blocks<LGO_PP>(c, maxb, 1, nullptr, Ki, n, npad, T, NB, w, gp);
    lgo_launch_blocks<LGO_BP>(c, maxb, (unsigned)d, hw.B, Ki, n, npad, T, NB, w, gp);
    hipLaunchKernelGGL(lgo_group_grad_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, gp,
                       lgo_chunks(npad), T, w.idx, w.start, w.sig, w.r, w.ar, hw.Z, d, npad, h, s, s2,
                       w.gpart);
    launch_fold(c, w.gpart, (int)G, d + 2, 1, d + 2, w.out + 1); // (gpart[group][d + 2])
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// ---- the posterior's derivatives in the hyper-parameters (ptheta.h; fit.hip, bq_gp_predict_dtheta) ----
static ThetaScale theta_scale(double h, double s)
{
    return ThetaScale{2.0 * (s * s) / h, -2.0 * s, 2.0 / h, 2.0 * s};
}

// R (64 x npad, ld 64) = [a, D_1 a .. D_d a] as rows, zero elsewhere
int launch_ptheta_dka(bq_ctx *c, int d, const HessJob &hj, double *R)
{
    if (bad_d_npad(d, hj.npad))
        return fail_d_npad(c, "ptheta_dka");
    Bracket br(c, BQ_K_REDUCE);
    BQ_DISPATCH_D(d, hipLaunchKernelGGL(ptheta_dka_kernel<D>, dim3((unsigned)hj.npad / 16), dim3(256),
                                        0, c->stream, hj, R));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// Row tile of the quad product, the one rule: the tall 256 x 64 tile (a quarter of the generated
// operand's exponentials per entry of beta) once its workgroups number at least one per CU and
// the rows it pads Mp with are at most a quarter of Mp (they are multiplied like any others: at
// Mp = 64 the tall tile does four times the flops), else 64 x 64 (four times the workgroups).
// BQ_GEMM_TILE=64|128 forces the small / the tall tile, as it forces the tiles of the gradient's
// and the Hessian's products (measurements, tests).
static bool ptheta_tall(const bq_ctx *c, int Mp, int npad)
{
    if (c->cfg.gemm_tile == 64 || c->cfg.gemm_tile == 128)
        return c->cfg.gemm_tile == 128;
    const long tiles = (Mp + 255) / 256;
    return tiles * (npad / 64) >= c->cus && 4 * (tiles * 256 - Mp) <= Mp;
}

size_t ptheta_part_doubles(int d, int Mp, int npad) { return (size_t)d * (npad / 64) * Mp; }

// part[k][npad / 64][Mp], k < d: the column blocks' pieces of q_jk = beta_j^T D_k beta_j, one launch
// per length scale
int launch_ptheta_quad(bq_ctx *c, int d, const double *beta, long ldb, int Mp, const HessJob &hj,
                       double *part)
{
    if (bad_d_npad(d, hj.npad) || (Mp % 64) || Mp < 64)
        return fail(c, BQ_ERR_BAD_ARG, "ptheta_quad: d in [1, %d], whole 64-blocks", BQ_MAXD);
    const bool tall = ptheta_tall(c, Mp, hj.npad);
    const unsigned gy = (unsigned)hj.npad / 64;
    for (int k = 0; k < d; ++k) {
        Bracket br(c, BQ_K_GEMM, 2.0 * Mp * (double)hj.n * hj.npad);
        BQ_DISPATCH_D(d, {
            if (tall)
                hipLaunchKernelGGL((ptheta_quad_kernel<D, 4, 1, 4, 4>),
                                   dim3((unsigned)(Mp + 255) / 256, gy), dim3(256), 0, c->stream,
                                   beta, ldb, Mp, hj, k, part);
            else
                hipLaunchKernelGGL((ptheta_quad_kernel<D, 2, 2, 2, 2>), dim3((unsigned)Mp / 64, gy),
                                   dim3(256), 0, c->stream, beta, ldb, Mp, hj, k, part);
        });
        HIPCHK(c, hipGetLastError());
    }
    return BQ_OK;
}

// dmean, dvar ((d + 2) x M, entry [p + j (d + 2)]) over the Mp (multiple of 16) rows of beta; a
// null dmean / dvar switches that part off (Z / beta, var and qpart are then not read)
int launch_predict_theta(bq_ctx *c, int d, const double *beta, long ldb, int M, int Mp,
                         const double *xo, const HessJob &hj, const double *Z, const double *var,
                         const double *qpart, double h, double s, double *dmean, double *dvar)
{
    Bracket br(c, BQ_K_REDUCE);
    const ThetaScale sc = theta_scale(h, s);
    const int ncb = hj.npad / 64;
    BQ_DISPATCH_D(d, hipLaunchKernelGGL(predict_theta_kernel<D>, dim3((unsigned)(Mp / 16)), dim3(512),
                                        0, c->stream, beta, ldb, M, xo, hj, Z, var, qpart, ncb,
                                        (long)Mp, sc, dmean, dvar));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// the fused mean route: mean (M; may be nullptr) and dmean ((d + 2) x M) in one launch
int launch_predict_mean_theta(bq_ctx *c, int d, const double *xo, int M, const HessJob &hj,
                              const double *Z, double h, double s, double *mean, double *dmean)
{
    Bracket br(c, BQ_K_REDUCE);
    const ThetaScale sc = theta_scale(h, s);
    BQ_DISPATCH_D(d, hipLaunchKernelGGL(predict_mean_theta_kernel<D>, dim3((unsigned)((M + 3) / 4)),
                                        dim3(256), 0, c->stream, xo, M, hj, Z, sc, mean, dmean));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

} // namespace bqh
