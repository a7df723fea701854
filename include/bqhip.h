/*
 * bqhip.h -- C ABI of libbqhip.so, the MI355X (gfx950) Bayesian-quadrature
 * GP engine.  This is the drop-in boundary: plain pointers and sizes, no
 * torch / numpy types.  The Python host package binds it with ctypes
 * (bayesian-quadrature_amd/_lib.py); INTEGRATION.md shows the stub a
 * maintainer of the reference would add.  The hardware probes are not part
 * of it: they live in libbqhip_probe.so (bqhip_probe.h).
 *
 * Reference interfaces replaced (jhamrick/bayesian-quadrature v0.2.0):
 *   bq_cho_factor      <- linalg_c.pyx:55-93   cho_factor(C, L)
 *   bq_cho_solve       <- linalg_c.pyx:96-179  cho_solve_vec / cho_solve_mat
 *   bq_logdet          <- linalg_c.pyx:182-210 logdet(L)
 *   bq_gram_gauss      <- gp.GP.Kxx / gp.GaussianKernel.__call__ (third-party
 *                         `gp` package, requirements.txt:2; used bq.py:147-162,465)
 *   bq_gp_fit          <- gp.GP.Lxx, .inv_Kxx_y, .log_lh   (bq.py:282,334-335,546)
 *   bq_gp_predict      <- gp.GP.mean(xo), diag(gp.GP.cov(xo)) (bq.py:200,227-228,942-943)
 *   bq_gp_logml_grid   <- the hyper-parameter loop body  (bq.py:536-550)
 *   bq_batch_fit_predict <- a Python loop over independent BQ problems
 *
 * Conventions
 *   - all floating point data is fp64; matrices are COLUMN-MAJOR (the
 *     reference's float64_t[::1, :]), points are d x n (gauss_c.pyx:116-117)
 *   - "host" pointers are caller-owned host memory; "_dev" entry points take
 *     device pointers obtained from bq_dev_alloc (or any HIP allocation on the
 *     context's device) and only enqueue work on the context's stream
 *   - every function returns a status code; bq_last_error() gives the text
 *   - a context is bound to one device and one stream and is not thread-safe;
 *     use one context per thread / per GPU
 */
#ifndef BQHIP_H
#define BQHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes; the Python layer maps them like linalg_c.pyx:49-53,88-91 */
#define BQ_OK 0
#define BQ_ERR_NOT_PD 1  /* dpotrf info > 0  -> numpy.linalg.LinAlgError */
#define BQ_ERR_BAD_ARG 2 /* shape / illegal value -> ValueError */
#define BQ_ERR_HIP 3     /* HIP runtime failure -> RuntimeError */
#define BQ_ERR_NOMEM 4   /* allocation failure -> MemoryError */

#define BQ_MAX_DIM 8 /* largest input dimension d */
#define BQ_LGO_MAX 64 /* largest group of bq_gp_lgo / bq_gp_lgo_grad */

typedef struct bq_ctx bq_ctx;
typedef struct bq_fit bq_fit;

/* ---- contexts ------------------------------------------------------ */
int bq_device_count(int *count);
int bq_ctx_create(int device, bq_ctx **out);
/* adopt an existing hipStream_t (e.g. a torch stream); not destroyed by us */
int bq_ctx_create_on_stream(int device, void *hip_stream, bq_ctx **out);
void bq_ctx_destroy(bq_ctx *ctx);
int bq_ctx_sync(bq_ctx *ctx);
const char *bq_last_error(const bq_ctx *ctx);
/* name: at least 64 bytes.  cus = compute units, hbm_bytes = total memory */
int bq_device_info(bq_ctx *ctx, char *name, int *cus, size_t *hbm_bytes, int *clock_khz);
/* outer Cholesky block (multiple of 64; 0 = automatic from the size) */
int bq_set_block(bq_ctx *ctx, int nb);
/* look-ahead of one panel on a second, high-priority stream (default on; the
 * environment variable BQ_LOOKAHEAD=0 also disables it) */
int bq_set_lookahead(bq_ctx *ctx, int on);
/* the look-ahead runs while the bulk trailing update still has at least `min_rows` rows;
 * below that the sweep continues with sequential launches (default 3072, the measured
 * cross-over on MI355X; 0 = look-ahead to the end; also BQ_LA_MIN) */
int bq_set_lookahead_rows(bq_ctx *ctx, int min_rows);
/* the three settings above as they stand (a caller that changes them for a while reads them
 * first and puts them back; any pointer may be NULL) */
int bq_get_config(bq_ctx *ctx, int *nb, int *lookahead, int *min_rows);
/* counters of the context since its creation, out[0 .. n): [0] single-vector solves that were
 * re-issued on the per-block sweeps after a hand-off of the one-launch sweeps timed out (the
 * call still returned BQ_OK with the right answer; non-zero on a healthy, unshared device means
 * something is wrong with it); [1] launch sequences captured into a hipGraph and instantiated
 * (a plan's pass, a pair's objective, a fit's single-vector sweeps); [2] launches of such graphs;
 * [3] graphs dropped because a setter had changed the configuration they were captured under
 * (the sequence is captured again at its next use).  [1]-[3] stay 0 with BQ_GRAPH=0.  Entries
 * beyond the ones defined are set to 0.  No reference
 * counterpart (linalg_c.pyx:96-136 is a LAPACK call) */
int bq_ctx_stats(bq_ctx *ctx, int64_t *out, int n);
/* bq_batch_fit_predict and bq_gp_logml_grid keep their device workspace (up to half of
 * the free HBM) in the context between calls, so that a hyper-parameter loop
 * (bq.py:536-550) does not allocate and release it on every evaluation; this releases it */
int bq_ctx_trim(bq_ctx *ctx);

/* ---- device memory -------------------------------------------------- */
int bq_dev_alloc(bq_ctx *ctx, size_t bytes, void **dptr);
int bq_dev_free(bq_ctx *ctx, void *dptr);
int bq_upload(bq_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);   /* synchronous */
int bq_download(bq_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes); /* synchronous */
int bq_memset(bq_ctx *ctx, void *dst_dev, int byte, size_t bytes);

/* ---- stream timers (HIP events on the context's stream) ------------- */
int bq_timer_start(bq_ctx *ctx);
int bq_timer_stop_ms(bq_ctx *ctx, float *ms); /* records, synchronises, returns elapsed */

/* per-kernel-class device time of everything enqueued since the last reset,
 * measured with HIP events around each launch (slows the pipeline: use in a
 * separate, instrumented pass).  Classes: */
#define BQ_K_GRAM 0       /* gram_gauss / assemble kernels            (work: bytes) */
#define BQ_K_POTF2 1      /* 64x64 diagonal factor                    (work: flop)  */
#define BQ_K_TRSM 2       /* panel solve                              (work: flop)  */
#define BQ_K_GEMM 3       /* in-panel (left-looking) MFMA update      (work: flop)  */
#define BQ_K_SYRK 4       /* trailing MFMA update, gemm_sub_kernel<4,4> launches    */
#define BQ_K_SYRK_SMALL 5 /* trailing MFMA update, the smaller-tile launches        */
#define BQ_K_REDUCE 6     /* finalize / reductions / predict          (work: bytes) */
#define BQ_K_NCLASS 7
int bq_profile_enable(bq_ctx *ctx, int on);
int bq_profile_reset(bq_ctx *ctx);
/* ms[BQ_K_NCLASS], launches[BQ_K_NCLASS], work[BQ_K_NCLASS] = the ALGORITHMIC flops
 * or bytes of the launches of each class (trailing update: the lower half only,
 * m^2 k; Gram: 8 N^2 + 8 d N); synchronises.  Any pointer may be NULL. */
int bq_profile_read(bq_ctx *ctx, double *ms, int64_t *launches, double *work);
/* the bracketed launches as a timeline: rows {class, stream (0 main / 1 second), start ms,
 * end ms, algorithmic work}, times since the first bracketed launch.  keep = 1 with out = NULL
 * arms (and clears) the recording; keep = 0 stops it -- with out = NULL that call only reports
 * *nrows, with out it copies up to max_rows rows. */
int bq_profile_timeline(bq_ctx *ctx, int keep, double *out, int64_t max_rows, int64_t *nrows);

/* ---- linalg_c drop-ins: host buffers in and out --------------------- */
/* L <- lower Cholesky factor of C (n x n, ld = n).  C == L allowed (in place).
 * The strict upper triangle of L is left as it was in C ("upper values could
 * be anything", linalg_c.pyx:58-59).  BQ_ERR_NOT_PD when dpotrf would fail;
 * *info (may be NULL) receives the 1-based failing column: the first column whose pivot is not a
 * positive finite number.  (A NaN or +inf pivot fails too, where LAPACK's dpotrf carries on; the
 * same rule holds for bq_potrf_dev's flag and for the status of the batched entry points.) */
int bq_cho_factor(bq_ctx *ctx, const double *C, double *L, int64_t n, int64_t *info);
/* X <- (L L^T)^-1 B, B and X are n x nrhs, ld = n.  B == X allowed. */
int bq_cho_solve(bq_ctx *ctx, const double *L, const double *B, double *X, int64_t n,
                 int64_t nrhs);
/* *out <- 2 sum_i log L[i,i] */
int bq_logdet(bq_ctx *ctx, const double *L, int64_t n, double *out);

/* ---- Gaussian-kernel Gram ------------------------------------------- */
/* K[i,j] = h^2 N(x_i | x_j, diag(w^2)) + s^2 [i==j]; full symmetric n x n
 * matrix, host in / host out.  x is d x n, w has d entries. */
int bq_gram_gauss(bq_ctx *ctx, const double *x, int64_t d, int64_t n, double h, const double *w,
                  double s, double *K_out);
/* same on device-resident data; only enqueues.  x_dev: d x n, K_dev: n x n
 * with leading dimension ldk >= n. */
int bq_gram_gauss_dev(bq_ctx *ctx, const double *x_dev, int64_t d, int64_t n, double h,
                      const double *w, double s, double *K_dev, int64_t ldk);
/* cross Gram K[i,j] = k(x1_i, x2_j), n1 x n2, host in / out (gp.GP.Kxxo, .K) */
int bq_gram_gauss_cross(bq_ctx *ctx, const double *x1, int64_t n1, const double *x2, int64_t n2,
                        int64_t d, double h, const double *w, double *K_out);

/* ---- device-resident Cholesky (the MFMA roofline path) -------------- */
/* In-place lower Cholesky of the n x n device matrix (ld = lda).  n must be a
 * multiple of 64 (callers pad with an identity block).  Only enqueues (the first call at a
 * new largest n also allocates 1024 n + 32768 bytes of panel scratch in the context); the
 * failing column (0 = success) is written to info_dev[0] (device int32). */
int bq_potrf_dev(bq_ctx *ctx, double *A_dev, int64_t n, int64_t lda, int32_t *info_dev);

/* ---- GP fit objects (device resident) ------------------------------- */
/* Fit a GP: Gram, Cholesky, z = L^-1 y, log marginal likelihood.  x is d x n
 * (host), y has n entries (host).  The factor stays on the device. */
int bq_gp_fit(bq_ctx *ctx, const double *x, const double *y, int64_t d, int64_t n, double h,
              const double *w, double s, bq_fit **out);
/* same data, new hyper-parameters (the hyper-parameter loop, bq.py:933-965) */
int bq_gp_refit(bq_ctx *ctx, bq_fit *fit, double h, const double *w, double s);
/* same points, new targets y (n entries, host): the hyper-parameter loop gives GP2 new targets
 * on every evaluation, `self.gp_l.y = self.l_sc`, bq.py:948-954.  The fit holds no valid factor
 * until its next bq_gp_refit / bq_gp_refit_predict. */
int bq_gp_set_y(bq_ctx *ctx, bq_fit *fit, const double *y);
/* new hyper-parameters and the posterior mean / marginal variance at M points xo (d x M, host)
 * in ONE sweep: the points ride as border rows of the fit's own bordered system.  This is the
 * body of the reference's hyper-parameter loop, bq.py:933-947 (`_set_gp_log_l_params`: set the
 * parameters, then gp.mean(x_c) and diag gp.cov(x_c)).  mean / var may be NULL (not both);
 * M > 63 falls back to bq_gp_refit + bq_gp_predict. */
int bq_gp_refit_predict(bq_ctx *ctx, bq_fit *fit, double h, const double *w, double s,
                        const double *xo, int64_t M, double *mean, double *var);
/* Append k observations (x_new: d x k column-major points, y_new: k targets) to a resident fit
 * under its current hyper-parameters.  Afterwards the handle is a fit of n + k points in every
 * respect.  O(k n^2): no Gram of the old points, no refactorisation.
 * BQ_ERR_NOT_PD: the Schur complement of the new points is not positive definite; the fit is
 * left exactly as it was (n, factor, z, log-ML, alpha: same bits).
 * BQ_ERR_BAD_ARG: stale fit ("refit required", as every consumer), null / k < 1 / non-finite. */
int bq_gp_append(bq_ctx *ctx, bq_fit *fit, const double *x_new, const double *y_new, int64_t k);
/* Remove the k observations idx[0 .. k) (distinct indices in [0, n), any order) from a resident fit
 * under its current hyper-parameters; the survivors keep their relative order.  Afterwards the
 * handle is a fit of n - k points in every respect.  O(k n^2) from the block column of the first
 * removed index on: no Gram, no refactorisation; removing the last k observations costs no
 * arithmetic on the factor at all.  A positive-semidefinite matrix is added to the compacted
 * factor's product, so there is no BQ_ERR_NOT_PD outcome.
 * BQ_ERR_BAD_ARG: stale fit ("refit required", as every consumer), null / k < 1 / k >= n / an index
 * out of range or given twice.  BQ_ERR_NOMEM / BQ_ERR_HIP: only from allocation, and before
 * anything is written: a failed call leaves the fit exactly as it was. */
int bq_gp_remove(bq_ctx *ctx, bq_fit *fit, const int64_t *idx, int64_t k);
void bq_fit_destroy(bq_ctx *ctx, bq_fit *fit);
int bq_gp_logml(bq_ctx *ctx, bq_fit *fit, double *out);
/* gradient of the fit's log marginal likelihood with respect to its hyper-parameters:
 * grad[0] = d/dh, grad[1..d] = d/dw_k, grad[d+1] = d/ds (host, d + 2 entries).
 * Same status rules as bq_gp_logml (stale / not-PD / null handle).  The first call after a
 * (re)fit builds L^-T: 2 npad^2 doubles of device memory, kept with the fit. */
int bq_gp_logml_grad(bq_ctx *ctx, bq_fit *fit, double *grad);
/* Hessian of the fit's log marginal likelihood with respect to its hyper-parameters, in the
 * gradient's order [h, w_1 .. w_d, s]: hess is (d + 2) x (d + 2) on the host, written in full,
 * hess[p][q] == hess[q][p] bit for bit.  Analytic: Kxx^-1 once and one n x n x n product per
 * length scale, nothing differenced.  Same status rules as bq_gp_logml_grad (stale / not-PD /
 * null handle or pointer; BQ_ERR_NOMEM when the workspace cannot be allocated, with nothing
 * half-made left behind).  The first call builds what the gradient keeps (L^-T) if it is not
 * there, and d npad^2 doubles of device memory more, kept with the fit; the result is kept until
 * the next (re)fit, bq_gp_set_y, bq_gp_append or bq_gp_remove.  The fit itself is not disturbed. */
int bq_gp_logml_hess(bq_ctx *ctx, bq_fit *fit, double *hess);
/* Leave-one-out cross-validation of the fit (Rasmussen & Williams 5.4.2): mean[i] and var[i] are
 * the predictive mean and variance of the noisy observation y_i (s^2 included) from the other
 * n - 1 observations, logpred[i] its log density at y_i, *total the sum of the logpred.  mean,
 * var, logpred: n doubles each on the host or NULL; total: one double or NULL; not all four NULL.
 * Closed form from diag Kxx^-1 and Kxx^-1 y: O(n^2) once L^-T is there (the gradient keeps it;
 * the first call builds it if not), nothing refitted.  Same status rules as bq_gp_logml_hess.
 * The same bits on every call and whichever of the gradient, the Hessian or bq_gp_loo_grad ran
 * before; kept until the next (re)fit, bq_gp_set_y, bq_gp_append or bq_gp_remove. */
int bq_gp_loo(bq_ctx *ctx, bq_fit *fit, double *mean, double *var, double *logpred,
              double *total);
/* Gradient of that total with respect to the hyper-parameters, in the order of bq_gp_logml_grad:
 * grad has d + 2 entries on the host (required); total: the value, or NULL.  Reads what the
 * Hessian keeps (Kxx^-1 and one n x n x n product per length scale: built here if no Hessian has
 * been taken since the fit last changed, and then not built again by bq_gp_logml_hess); beyond
 * that O((d + 1) n^2).  Device memory: the Hessian's, and (d + 5) npad doubles and partial sums
 * more, all allocated before anything runs: BQ_ERR_NOMEM leaves the fit as it was. */
int bq_gp_loo_grad(bq_ctx *ctx, bq_fit *fit, double *total, double *grad);
/* Leave-group-out cross-validation: whole groups of observations left out at once (a cluster of
 * close samples, a block, a fold).  Group g is idx[start[g] .. start[g + 1]), start[0] = 0,
 * T = start[G]; the groups are disjoint, hold 1 .. BQ_LGO_MAX indices each and need not cover the
 * fit (a point in no group is never left out).  mean and var (T doubles each, in the order of
 * idx): the predictive mean and variance of the noisy observation (s^2 included; the diagonal of
 * the group's predictive covariance) from the points outside its group; logpred (G doubles): the
 * joint log density of each group at its targets; *total: their sum.  Any output may be NULL, not
 * all four.  Closed form from the groups' blocks of Kxx^-1 and Kxx^-1 y: O(n b^2) per group of b
 * once L^-T is there, nothing refitted.  BQ_ERR_BAD_ARG: a stale fit, G < 1, an empty group or one
 * above the cap, an index out of range or given twice; BQ_ERR_NOT_PD: a block of Kxx^-1 with a
 * pivot that is not positive and finite, and then no output is written.  The same bits on every
 * call, whatever ran before; nothing is kept between calls but the workspace, allocated before
 * anything runs (BQ_ERR_NOMEM leaves the fit as it was). */
int bq_gp_lgo(bq_ctx *ctx, bq_fit *fit, const int64_t *idx, const int64_t *start, int64_t G,
              double *mean, double *var, double *logpred, double *total);
/* Gradient of that total with respect to the hyper-parameters, in the order of bq_gp_logml_grad:
 * grad has d + 2 entries on the host (required); total: the value, bit for bit bq_gp_lgo's, or
 * NULL.  Reads the Hessian's products stage as bq_gp_loo_grad does (built here if it is not
 * there, and then kept for the Hessian and bq_gp_loo_grad); beyond that O((d + 1) n b^2) per
 * group. */
int bq_gp_lgo_grad(bq_ctx *ctx, bq_fit *fit, const int64_t *idx, const int64_t *start, int64_t G,
                   double *total, double *grad);
/* which: 0 = L (n x n, strict upper zeroed), 1 = alpha = Kxx^-1 y (n),
 * 2 = z = L^-1 y (n), 3 = Kxx (n x n, recomputed) */
int bq_gp_get(bq_ctx *ctx, bq_fit *fit, int which, double *out_host);
/* posterior at M points xo (d x M, host): mean[M], var[M] (marginal, prior
 * scale minus explained part; either may be NULL), cov (M x M full posterior
 * covariance, may be NULL). */
int bq_gp_predict(bq_ctx *ctx, bq_fit *fit, const double *xo, int64_t M, double *mean,
                  double *var, double *cov);
/* The posterior at M points and its gradients with respect to the points themselves, in closed
 * form on the resident factor (nothing differenced, nothing refitted):
 *   d mean_j / d xo_jk =      sum_i k(xo_j, x_i) (x_ik - xo_jk) / w_k^2 alpha_i,  alpha  = Kxx^-1 y
 *   d var_j  / d xo_jk = -2   sum_i k(xo_j, x_i) (x_ik - xo_jk) / w_k^2 beta_ji,  beta_j = Kxx^-1 k_j
 * xo: d x M column-major like bq_gp_predict.  mean, var: M.  dmean, dvar: d x M, entry [k + j*d] =
 * d/d xo_jk.  Any output may be NULL, not all four.  Without var and dvar: one fused launch, no
 * sweep.  Otherwise the sweep of bq_gp_predict -- mean and var are its bits -- and, for dvar, one
 * backward row sweep more; O(M n^2) like the prediction itself.  Same status rules as
 * bq_gp_predict, and BQ_ERR_BAD_ARG when all four outputs are NULL; M == 0 touches nothing.  The
 * same bits on every call; the fit is not disturbed.  Workspaces are bq_gp_predict's, kept with
 * the fit. */
int bq_gp_predict_grad(bq_ctx *ctx, bq_fit *fit, const double *xo, int64_t M, double *mean,
                       double *var, double *dmean, double *dvar);
/* The posterior at M points and its derivatives with respect to the hyper-parameters
 * theta = [h, w_1 .. w_d, s] (the order of bq_gp_logml_grad), in closed form on the resident factor:
 * nothing differenced, nothing refitted, no cached result of the fit dropped.  With a = Kxx^-1 y,
 * beta_j = Kxx^-1 k_j, u = Kxx^-1 a, z_k = Kxx^-1 (D_k a), D_k = d Kxx / d w_k and
 * g_jik = (xo_jk - x_ik)^2 / w_k^3 - 1 / w_k:
 *   d mean_j / d h = (2 s^2 / h) k_j.u    d mean_j / d w_k = sum_i k_ji (g_jik a_i - z_k,i)
 *   d mean_j / d s = -2 s k_j.u
 *   d var_j / d h = (2 / h)(var_j - s^2 |beta_j|^2)     d var_j / d s = 2 s |beta_j|^2
 *   d var_j / d w_k = -k(x, x) / w_k - 2 sum_i k_ji g_jik beta_ji + beta_j^T D_k beta_j
 * xo: d x M column-major like bq_gp_predict.  mean, var: M.  dmean, dvar: (d + 2) x M, entry
 * [p + j*(d + 2)] = d/d theta_p.  Any output may be NULL, not all four.  Without var and dvar: one
 * fused launch, no sweep.  Otherwise the sweep of bq_gp_predict -- mean and var are its bits --
 * and, for dvar, one backward row sweep and one M x n x n product per length scale.  u and z_k
 * are solved once per fit and kept until it changes.  Same status rules as bq_gp_predict, and
 * BQ_ERR_BAD_ARG when all four outputs are NULL; M == 0 touches nothing.  The same bits on every
 * call.  At s == 0 the h entry of dmean and the s entries of both are exactly 0. */
int bq_gp_predict_dtheta(bq_ctx *ctx, bq_fit *fit, const double *xo, int64_t M, double *mean,
                         double *var, double *dmean, double *dvar);
/* The polynomial trend of a fit, its coefficients marginalised (universal kriging; Rasmussen &
 * Williams 2.7): y = phi(x)^T beta + f(x) + eps with f the fit's zero-mean GP and a flat prior on
 * beta, which is integrated out.  A stateless view of the fit like bq_gp_loo or bq_gp_sample: the
 * fit itself stays zero-mean for every other entry point.
 * The basis is fixed by degree in {0, 1, 2}, a centre c and a scale rho (d entries each, finite,
 * rho_k > 0).  With t = (x - c) / rho the columns of phi(x) are, in this order: 1; for degree >= 1
 * t_1 .. t_d; for degree 2 t_k t_l for k = 1 .. d, l = k .. d (k outer) -- p = 1, 1 + d or
 * 1 + d + d (d + 1) / 2 of them, at most 45.  Centring and scaling are part of the contract: they
 * are what keeps H^T Kxx^-1 H well conditioned.
 * With H (n x p, rows phi(x_i)^T), L L^T = Kxx, z = L^-1 y, G = L^-1 H, A = G^T G, b = G^T z:
 *   beta     = A^-1 b                                  cov_beta = A^-1
 *   alpha_t  = Kxx^-1 (y - H beta) = L^-T (z - G beta)   (so that H^T alpha_t = 0)
 *   logml_t  = -1/2 (|z|^2 - b^T beta) - 1/2 log|Kxx| - 1/2 log|A| - 1/2 (n - p) log 2 pi
 * logml_t is R&W (2.45) for a flat prior.  Its log|A| term is that of the SCALED basis: an
 * improper prior leaves an additive constant free, and another (c, rho) of the same degree moves
 * logml_t by log|det| of the change of basis -- compare values of one basis only.
 * Host outputs: beta (p), cov_beta (p x p column-major), logml_t (one value), alpha_t (n).  Any
 * may be NULL, not all four.
 * Status rules of bq_gp_predict for the handle; BQ_ERR_BAD_ARG for a degree outside 0 .. 2, a
 * centre that is not finite, a scale that is not finite and positive, n < p -- all checked before
 * anything is allocated; BQ_ERR_NOT_PD when a pivot of A is not positive and finite, and then no
 * output is written.  One row sweep of 64 rows over the resident factor, slices of A and b folded
 * in a fixed order, one workgroup for the p x p system, one single-vector sweep: O(p n^2).  The
 * result is kept with the fit for the key (degree, c, rho) until the factor or the targets change;
 * a call with another key recomputes it.  Device memory (130 npad doubles and the partial sums,
 * kept with the fit) is allocated before anything is enqueued: BQ_ERR_NOMEM leaves the fit as it
 * was.  The fit is not disturbed; the same inputs give the same bits on every call, whether or
 * not the state was there and whatever ran before. */
int bq_gp_trend(bq_ctx *ctx, bq_fit *fit, int degree, const double *center, const double *scale,
                double *beta, double *cov_beta, double *logml_t, double *alpha_t);
/* The posterior of that model at M points xo (d x M column-major like bq_gp_predict).  With
 * v_j = L^-1 k(x, xo_j) and r_j = phi(xo_j) - G^T v_j:
 *   mean_j = v_j.z + r_j.beta                    (= k_j^T alpha_t + phi(xo_j)^T beta)
 *   var_j  = k(x, x) - |v_j|^2 + r_j^T A^-1 r_j  (latent, like bq_gp_predict's var)
 * -- the last term carries the uncertainty of the coefficients, so var_j >= bq_gp_predict's.
 * mean and var (M each) may be NULL, not both.  Without var: one fused launch over alpha_t, no
 * sweep.  With it: the cross Gram and sweep of bq_gp_predict; the p sums v_j.G_k ride in its row
 * reductions' one pass over V for p <= 8 (v_j.z and |v_j|^2 are then bq_gp_predict's bits), and
 * are one product more beyond; p^2 flops per point finish.  The state of bq_gp_trend is used when
 * it is there for this key and computed (and kept) when it is not: either way everything is
 * enqueued without waiting for the device and read back once, the bits are the same, and nothing
 * reaches the caller's memory on BQ_ERR_NOT_PD.  Arguments and statuses as bq_gp_trend, and
 * BQ_ERR_BAD_ARG for M < 0 or mean == var == NULL; M == 0 touches nothing.  Workspaces are
 * bq_gp_predict's and 64 M doubles, kept with the fit. */
int bq_gp_predict_trend(bq_ctx *ctx, bq_fit *fit, int degree, const double *center,
                        const double *scale, const double *xo, int64_t M, double *mean,
                        double *var);
/* The route the fit's last bq_gp_predict_trend took (tests): *route = 0 the fused mean launch, 1
 * the one-pass row reductions, 2 the product (then *gemm_kernel, if given, is the product's
 * kernel as launch_gemm numbers them; else -1); -1 before the first call. */
int bq_gp_trend_last_route(bq_ctx *ctx, bq_fit *fit, int *route, int *gemm_kernel);
/* S joint draws of the latent posterior at M points, on the device: the sweep of bq_gp_predict,
 * Sigma = K(xo, xo) - V V^T (no s^2: the matrix bq_gp_predict returns as cov), its device Cholesky
 * factor and one triangular product:
 *   out[:, s] = mean + L_c z_s,   L_c L_c^T = Sigma + jitter I.
 * xo: d x M column-major like bq_gp_predict.  out: M x S column-major on the host (required).
 * z: M x S column-major standard normals of the caller's, or NULL: then element e = j + M s is drawn
 * on the device from Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (e & 0xffffffff, e >> 32, 0, 0), outputs r0 .. r3:
 *   u1 = ((r0 >> 5) 2^26 + (r1 >> 6) + 1) 2^-53,  u2 = ((r2 >> 5) 2^26 + (r3 >> 6)) 2^-53,
 *   z = sqrt(-2 ln u1) cos(2 pi u2)
 * -- a value depends on (seed, e) alone, so a host program can reproduce it.  seed is ignored when
 * z is given.
 * ladder: nl >= 1 finite multiples of k0 = k(x, x), the prior variance, tried in order on the one
 * Sigma that was formed; the first whose Sigma + k0 ladder[t] I factors is used (entries may be
 * negative).  NULL: the default ladder 0, 1e-12, 1e-10, 1e-8, 1e-6 (nl is ignored).  A smooth
 * posterior at dense points is numerically singular: the jitter is part of the contract.
 * mean (M, or NULL): the bits bq_gp_predict returns when asked for mean and var.  chol (M x M
 * column-major, or NULL): L_c, its strict upper triangle exact zeros.  jitter (one double, or
 * NULL): the absolute value added, k0 ladder[t].
 * Status rules of bq_gp_predict for the handle; BQ_ERR_BAD_ARG for M < 0, S < 1,
 * M > BQ_SAMPLE_MAX_M, S > BQ_SAMPLE_MAX_S, out == NULL, a ladder entry that is not finite, nl < 1
 * with a ladder -- all checked before anything is allocated; M == 0 touches nothing.
 * BQ_ERR_NOT_PD: every ladder entry failed; no output is written.  Device memory (the prediction's
 * workspaces, one or two Mp x Mp matrices and two Mp x S ones, Mp = M rounded up to 64; kept with
 * the fit) is allocated before anything is enqueued: BQ_ERR_NOMEM leaves the fit as it was.  The
 * fit is not disturbed; the same inputs give the same bits on every call, and column s of out does
 * not depend on S. */
#define BQ_SAMPLE_MAX_M 16384
#define BQ_SAMPLE_MAX_S 4096
int bq_gp_sample(bq_ctx *ctx, bq_fit *fit, const double *xo, int64_t M, int64_t S,
                 const double *z, uint64_t seed, const double *ladder, int64_t nl,
                 double *out, double *mean, double *chol, double *jitter);
/* The greedy, diagonally pivoted partial Cholesky factorisation of the latent posterior
 * covariance Sigma = K(xo, xo) - V V^T (no s^2: the matrix bq_gp_predict returns as cov) at M
 * points, on the device and without forming Sigma: the sweep of bq_gp_predict, then at most q
 * steps.  xo: d x M column-major like bq_gp_predict.  nugget >= 0 in absolute units; tol >= 0 in
 * multiples of k0 = k(x, x), the prior variance (as bq_gp_sample's ladder is).
 * With d^(0) = diag Sigma (the var bq_gp_predict returns less s^2), for j = 0 .. q - 1:
 *   p_j    = argmax_i d^(j)_i over the M points, the lowest index among equals;
 *   gain_j = d^(j)[p_j]; the factorisation ends with rank = j when gain_j <= tol k0, when
 *            gain_j <= 0 or when it is not finite -- no step divides by a non-positive number;
 *   c_j    = (K(xo, xo_{p_j}) - V V[p_j, :]^T - sum_{i<j} c_i c_i[p_j]) / sqrt(gain_j + nugget);
 *   d^(j+1) = d^(j) - c_j o c_j.
 * The pivots are the max-variance sequential design.  With L the q x q lower triangle of
 * C[piv, :] whose diagonal is sqrt(gain_j + nugget), L L^T = Sigma[piv, piv] + nugget I and
 * C L^T = Sigma[:, piv], so that d^(rank) = diag(Sigma - Sigma[:, P] (Sigma[P, P] + nugget I)^-1
 * Sigma[P, :]): with nugget = s^2 the posterior variances after noisy observations at the chosen
 * points, whatever their targets.  C[p_j, j] itself is gain_j / sqrt(gain_j + nugget).
 * nugget == 0: C[p_j, j] = sqrt(gain_j) and L = C[piv, :], lower triangular; a taken row keeps
 * d = 0 exactly, stores an exact 0 in every later column and is never taken twice.  nugget > 0: a
 * row may be taken again (two noisy observations at one place) and nothing is zeroed.
 * Outputs on the host: piv (q, -1 from rank on), gain (q, 0 from rank on) and rank (one value) are
 * required; C (M x q column-major, zero columns from rank on) and resid (M: d^(rank)) may be NULL.
 * The same inputs give the same bits on every call, and the first j pivots, gains and columns of
 * a q-step call are bit for bit those of a j-step call.
 * Status rules of bq_gp_predict for the handle; BQ_ERR_BAD_ARG for M < 0, q < 1, q > M (but for
 * M == 0), M > BQ_PIVCHOL_MAX_M, q > BQ_PIVCHOL_MAX_Q, a negative or non-finite nugget or tol, or
 * piv, gain or rank == NULL -- all checked before anything is allocated.  M == 0 writes rank = 0,
 * piv = -1 and gain = 0 and touches nothing else.  The limits: M rounded up to 64 makes at most
 * 16384 row blocks, which every kernel of the sweep and of the steps holds in any grid dimension,
 * and the steps' slices of the npad + q columns stay below a grid's second dimension; offsets into
 * the M x (N + q) matrix are 64-bit throughout.  Device memory (the prediction's workspaces with
 * q more columns, Mp (1 + slices) doubles more; kept with the fit) is allocated before anything
 * is enqueued: BQ_ERR_NOMEM leaves the fit as it was.  All steps are enqueued without waiting
 * for the device; nothing reaches the caller's memory unless every kernel has completed.  The
 * fit is not disturbed. */
#define BQ_PIVCHOL_MAX_M 1048576
#define BQ_PIVCHOL_MAX_Q 65536
int bq_gp_pivchol(bq_ctx *ctx, bq_fit *fit, const double *xo, int64_t M, int64_t q, double nugget,
                  double tol, int64_t *piv, double *C, double *resid, double *gain, int64_t *rank);
/* The greedy design that minimises the integrated posterior variance (integrated variance
 * reduction; ALC, IMSPE): which q of A candidates xc (d x A column-major) to observe so that
 * sum_j rho_j var(r_j) over R reference points xr (d x R) with weights rho (R, finite, >= 0)
 * drops the most, one point at a time.  The reference points and weights describe the measure the
 * variance is integrated against: a grid or a sample of it.  On the device, after one sweep of
 * bq_gp_predict over the joint point set.  Sigma is the latent posterior covariance (no s^2) over
 * [xr | xc]; nugget >= 0 in absolute units is an observation's noise; tol >= 0 in multiples of
 * k0 sum_j rho_j, k0 = k(x, x).
 * With T = Sigma(xc, xr) (A x R), dc = diag Sigma(xc, xc), dr = diag Sigma(xr, xr) and
 * ivar0 = sum_j rho_j dr[j], for t = 0 .. q - 1:
 *   eligible  a candidate with dc[a] + nugget > 0 that, when nugget == 0, has not been taken;
 *   score[a] = (sum_j rho_j T[a, j]^2) / (dc[a] + nugget): exactly the drop of sum_j rho_j dr[j]
 *             when xc_a is observed with noise nugget;
 *   p_t      = the eligible candidate with the largest score, the lowest index among equals; a
 *             NaN score comes first;
 *   gain_t   = score[p_t]; the run ends with rank = t unless gain_t > tol k0 sum rho, is positive
 *             and is finite;
 *   c        = (K(xc, xc_p) - V_c V_c[p]^T - sum_{i<t} c_i c_i[p]) / sqrt(dc[p] + nugget),
 *   u        = T[p, :] / sqrt(dc[p] + nugget);
 *   T -= c u^T, dc -= c o c, dr -= u o u (each entry one fma).
 * nugget == 0: c[p] = sqrt(dc[p]), a taken candidate keeps dc = 0 exactly, has c = 0 from then on
 * and is never taken twice.  nugget > 0: a candidate may be taken again (two noisy observations
 * at one place).  So sum_j rho_j dr^(t+1)[j] = sum_j rho_j dr^(t)[j] - gain_t, and with
 * nugget = s^2 the final dr and dc are the variances a fit has at xr and xc after bq_gp_append of
 * the chosen points, whatever their targets.  Step 0's scores are the acquisition surface.
 * xr == NULL with R == 0: the candidates are the reference points, rho has A entries, one sweep
 * runs over the A points (not over two copies of them), dr is dc, and resid_r, if given, receives
 * the same A values as resid_c.
 * Outputs on the host: piv (q, -1 from rank on), gain (q, 0 from rank on), ivar0 and rank (one
 * value each) are required; resid_r (R: dr after the last step), resid_c (A: dc) and score0 (A:
 * step 0's scores, 0 where a candidate is not eligible) may be NULL.
 * The same inputs give the same bits on every call, and the first j pivots and gains of a q-step
 * call are bit for bit those of a j-step call.
 * Status rules of bq_gp_predict for the handle; BQ_ERR_BAD_ARG for A < 0, R < 0, q < 1, q > A (but
 * for A == 0), R + A > BQ_PIVCHOL_MAX_M, q > BQ_PIVCHOL_MAX_Q, more than BQ_IVR_MAX_CELLS entries
 * of T (A and R each rounded up to 64), a negative or non-finite nugget, tol or weight, xr == NULL
 * with R > 0 or the reverse, or piv, gain, ivar0, rank or -- unless A == 0 -- rho or xc == NULL:
 * all checked before anything is allocated, and nothing is written.  A == 0 writes rank = 0,
 * piv = -1, gain = 0 and ivar0 = 0 and touches nothing else.  Device memory (T; the prediction's
 * workspaces over R + A points with q more columns; a few vectors; kept with the fit) is
 * allocated before anything is enqueued: BQ_ERR_NOMEM leaves the fit as it was.  All steps are
 * enqueued without waiting for the device; nothing reaches the caller's memory unless every
 * kernel has completed.  The fit is not disturbed. */
#define BQ_IVR_MAX_CELLS 268435456
int bq_gp_ivr(bq_ctx *ctx, bq_fit *fit, const double *xr, int64_t R, const double *rho,
              const double *xc, int64_t A, int64_t q, double nugget, double tol, int64_t *piv,
              double *gain, double *ivar0, double *resid_r, double *resid_c, double *score0,
              int64_t *rank);
/* Vanilla Bayesian quadrature of a resident fit: the posterior of Z = int f(x) N(x | mu, Sigma) dx
 * under the fit's GP.  mu: d; cov: Sigma, d x d symmetric positive definite, column-major, as
 * bq_int_K takes them.  With k = h^2 N(. | ., diag(w^2)), Kxx = K + s^2 I = L L^T, z = L^-1 y,
 *   kappa(x) = int k(x, x') N(x' | mu, Sigma) dx' = h^2 N(x | mu, diag(w^2) + Sigma)  (bq_int_K),
 *   kk       = int int k N N                      = h^2 N(0 | 0, diag(w^2) + 2 Sigma),
 *   kappa_X  = kappa at the fit's points,  b = L^-1 kappa_X:
 *   *mean   = b . z;
 *   *var    = kk - b . b: latent, like bq_gp_predict's variance, and like it NOT clamped at 0 -- the
 *             project's variance reductions subtract and store, so rounding may leave a variance
 *             of a few ulp of kk below 0;
 *   weights = L^-T b = Kxx^-1 kappa_X (n doubles): the quadrature weights, mean = weights . y.
 * Any output may be NULL, but not all three.  kappa_X, b, b.b and kk are kept with the fit for
 * the measure they were computed for: a call with the same (mu, Sigma) costs one dot product b.z
 * against the current z (and one single-vector backward sweep for the weights); a call with
 * another measure recomputes them (int_K_kernel on the resident points, one single-vector
 * forward sweep, one reduction -- enqueued without waiting, one read-back).  A refit, an append and
 * a removal discard them; new targets do not, since b does not depend on y.
 * Status rules of bq_gp_predict for the handle; BQ_ERR_BAD_ARG for mu or cov == NULL, all three
 * outputs NULL, a non-finite entry of mu or cov, or a diag(w^2) + Sigma (or + 2 Sigma) that is
 * not positive definite -- all checked before anything is allocated, and nothing is written. */
int bq_gp_integral(bq_ctx *ctx, bq_fit *fit, const double *mu, const double *cov, double *mean,
                   double *var, double *weights);
/* The greedy design that minimises the posterior variance of the integral Z of bq_gp_integral
 * (sequential Bayesian quadrature, Huszar & Duvenaud 2012): which q of A candidates xc (d x A
 * column-major) to observe so that var Z drops the most, one point at a time.  Every ingredient is
 * closed form: no reference points stand for the measure.  On the device, after one sweep of
 * bq_gp_predict over the candidates.  Sigma_c is the latent posterior covariance (no s^2) over xc
 * with v_a = L^-1 k(x, xc_a) the rows of the sweep's V; nugget >= 0 in absolute units is an
 * observation's noise; tol >= 0 in multiples of kk, the prior variance of Z.
 * With dc = diag Sigma_c (bq_gp_predict's variance bits), u_a = kappa(xc_a) - v_a . b =
 * Cov(Z, f(xc_a) | data) and *zvar0 = bq_gp_integral's var, for t = 0 .. q - 1:
 *   eligible  a candidate with dc[a] + nugget > 0 that, when nugget == 0, has not been taken;
 *   score[a] = u_a^2 / (dc[a] + nugget): exactly the drop of var Z when xc_a is observed with noise
 *             nugget;
 *   p_t      = the eligible candidate with the largest score, the lowest index among equals; a
 *             NaN score comes first;
 *   gain_t   = score[p_t]; the run ends with rank = t unless gain_t > tol kk, is positive and is
 *             finite;
 *   den      = sqrt(dc[p] + nugget),
 *   c        = (K(xc, xc_p) - V V[p]^T - sum_{i<t} c_i c_i[p]) / den;
 *   u -= c (u_p / den), dc -= c o c (each entry one fma).
 * nugget == 0: c[p] = den, a taken candidate keeps dc = 0 and u = 0 exactly, has c = 0 from then
 * on and is never taken twice.  nugget > 0: a candidate may be taken again (two noisy observations
 * at one place) and nothing is zeroed.  So var Z after t steps is zvar0 - sum_{i<t} gain_i, and
 * with nugget = s^2 that is the var bq_gp_integral returns after bq_gp_append of the chosen points,
 * whatever their targets.  Step 0's scores are the acquisition surface.
 * Outputs on the host: piv (q, -1 from rank on), gain (q, 0 from rank on), zvar0 and rank (one
 * value each) are required; resid_u (A: u after the last step), resid_c (A: dc) and score0 (A:
 * step 0's scores, 0 where a candidate is not eligible) may be NULL.
 * The same inputs give the same bits on every call, and the first j pivots and gains of a q-step
 * call are bit for bit those of a j-step call.
 * Status rules of bq_gp_predict for the handle; BQ_ERR_BAD_ARG as in bq_gp_integral for mu and
 * cov, and for A < 0, q < 1, q > A (but for A == 0), A > BQ_PIVCHOL_MAX_M, q > BQ_PIVCHOL_MAX_Q, a
 * negative or non-finite nugget or tol, or piv, gain, zvar0, rank or -- unless A == 0 -- xc ==
 * NULL: all checked before anything is allocated, and nothing is written.  A == 0 writes
 * rank = 0, piv = -1, gain = 0 and zvar0 and touches nothing else.  Device memory (the prediction's
 * workspaces with q more columns, Ap (5 + slices) doubles more; kept with the fit) is allocated
 * before anything is enqueued: BQ_ERR_NOMEM leaves the fit as it was.  All steps are enqueued
 * without waiting for the device; nothing reaches the caller's memory unless every kernel has
 * completed.  The fit is not disturbed; bq_gp_integral's state for (mu, Sigma) is computed on the
 * way where it is not there. */
int bq_gp_zdesign(bq_ctx *ctx, bq_fit *fit, const double *mu, const double *cov, const double *xc,
                  int64_t A, int64_t q, double nugget, double tol, int64_t *piv, double *gain,
                  double *zvar0, double *resid_u, double *resid_c, double *score0, int64_t *rank);
/* bq_gp_integral and bq_gp_zdesign under two more measures.  Everything but kappa and kk is those
 * two contracts word for word: b = L^-1 kappa_X, mean = b . z, var = kk - b . b not clamped, the
 * weights, u_a = kappa(xc_a) - v_a . b, the recurrence with its stop, tie and NaN rules, the
 * outputs that may be NULL, what is allocated when, and the state kept with the fit -- one state,
 * for the measure of the last call, whatever its kind: a measure of another kind, or other numbers
 * of the same kind, recomputes it.  A box and a Gaussian with the same numbers are two measures.
 *
 * The uniform measure on the box prod_k [lo_k, hi_k] (lo, hi: d doubles each), density 1 / vol.
 * With L_k = hi_k - lo_k and Phi the standard normal distribution function:
 *   kappa(x) = h^2 prod_k (Phi((hi_k - x_k) / w_k) - Phi((lo_k - x_k) / w_k)) / L_k,
 *   kk       = h^2 prod_k (L_k erf(L_k / (sqrt2 w_k)) + w_k sqrt(2 / pi) expm1(-L_k^2 / (2 w_k^2)))
 *              / L_k^2.
 * The difference of the two Phi is taken from erfc on the side of x_k where both ends lie, and as a
 * sum of two erf where x_k lies between them: no cancellation in either tail.
 * BQ_ERR_BAD_ARG, beyond the Gaussian entry point's: lo or hi == NULL, a non-finite entry, or
 * lo_k >= hi_k.
 *
 * The mixture sum_c pi_c N(mu_c, Sigma_c), c < C <= BQ_MEASURE_MAX_COMP.  pi: C weights, finite,
 * >= 0 and not all zero, used as given and NOT normalised; mu: d x C column-major; cov: C
 * column-major d x d blocks, each symmetric, any of which may be zero (a point mass at mu_c: an
 * empirical measure is a mixture of those).
 *   kappa(x) = sum_c pi_c h^2 N(x | mu_c, diag(w^2) + Sigma_c)               in ascending c,
 *   kk       = sum_c sum_c' pi_c pi_c' h^2 N(mu_c - mu_c' | 0, diag(w^2) + Sigma_c + Sigma_c')
 *                                                                  in ascending c, then c'.
 * Each component is evaluated as bq_int_K evaluates its measure; the first term of a sum is the
 * plain product and every later one a single fma.  So C = 1 with pi = 1 gives the bits of the
 * Gaussian entry point in every output.
 * BQ_ERR_BAD_ARG, beyond the Gaussian entry point's: pi, mu or cov == NULL, C < 1 or C >
 * BQ_MEASURE_MAX_COMP, a non-finite entry, a negative weight, weights that sum to zero, or a
 * diag(w^2) + Sigma_c or diag(w^2) + Sigma_c + Sigma_c' that is not positive definite.
 * All of it is checked before anything is allocated, and nothing is written. */
#define BQ_MEASURE_MAX_COMP 64
int bq_gp_integral_box(bq_ctx *ctx, bq_fit *fit, const double *lo, const double *hi, double *mean,
                       double *var, double *weights);
int bq_gp_integral_mix(bq_ctx *ctx, bq_fit *fit, int64_t C, const double *pi, const double *mu,
                       const double *cov, double *mean, double *var, double *weights);
int bq_gp_zdesign_box(bq_ctx *ctx, bq_fit *fit, const double *lo, const double *hi,
                      const double *xc, int64_t A, int64_t q, double nugget, double tol,
                      int64_t *piv, double *gain, double *zvar0, double *resid_u, double *resid_c,
                      double *score0, int64_t *rank);
int bq_gp_zdesign_mix(bq_ctx *ctx, bq_fit *fit, int64_t C, const double *pi, const double *mu,
                      const double *cov, const double *xc, int64_t A, int64_t q, double nugget,
                      double tol, int64_t *piv, double *gain, double *zvar0, double *resid_u,
                      double *resid_c, double *score0, int64_t *rank);
/* The marginal of a resident fit: some axes integrated, the others kept.  keep: d flags, 1 for a
 * kept axis (the set S, 1 <= |S| <= d - 1), 0 for an integrated one (I).  For a measure pi on all
 * d axes,
 *   J(q) = int f(q, t) pi(q, t) dt,   q on the kept axes, t on the integrated ones,
 * the UNNORMALISED marginal: int J(q) dq is bq_gp_integral's Z, the double integral of its
 * covariance is var Z, and J / Z is the marginal posterior density.  J is linear in f, hence a
 * Gaussian process in closed form: with k(x, x') = h^2 prod_k N(x_k | x'_k, w_k^2), W_S and W_I
 * the blocks of diag(w^2) and v_q = L^-1 c(q, X)^T,
 *   mean(q) = c(q, X) alpha,  cov(q, q') = P(q, q') - v_q . v_q',  var(q) = P(q, q) - |v_q|^2,
 * latent and not clamped, like every variance here.
 *
 * bq_gp_marginal: the Gaussian N(mu, Sigma) of bq_gp_integral (mu: d, cov: d x d column-major,
 * finite and symmetric).  With B = Sigma_IS Sigma_SS^-1, m(q) = mu_I + B (q - mu_S), Sigma_c =
 * Sigma_II - B Sigma_SI and pi_S(q) = N(q | mu_S, Sigma_SS):
 *   c(q, x_j) = h^2 pi_S(q) N(q | x_jS, W_S) N(x_jI | m(q), W_I + Sigma_c),
 *   P(q, q')  = h^2 N(q | q', W_S) pi_S(q) pi_S(q') N(m(q) - m(q') | 0, W_I + 2 Sigma_c).
 * Every entry is one exponential of the summed exponents: no density underflows on its own.
 * bq_gp_marginal_box: the uniform measure on prod_k [lo_k, hi_k] of bq_gp_integral_box.  With
 * kappa_box,I and kk_box,I that entry point's kappa and kk over the integrated axes alone (h^2
 * included) and vol_S the volume of the kept axes' box:
 *   c(q, x_j) = 1[q in box_S] / vol_S   N(q | x_jS, W_S) kappa_box,I(x_jI),
 *   P(q, q')  = 1[q, q' in box_S] / vol_S^2 N(q | q', W_S) kk_box,I.
 * The closed box counts as inside; a q outside gives exact zeros in mean, var and its row and
 * column of cov.  There is no entry point for a mixture (its conditional has weights that depend
 * on q), none for the square-root-warped model, and no design that lowers a marginal's variance.
 *
 * xq: d x M column-major like bq_gp_predict's xo; the coordinates of integrated axes are never
 * read.  mean, var: M; cov_out: M x M column-major; any may be NULL, not all.  Mean alone takes a
 * fused route (alpha, one launch, no matrix); anything else the forward sweep of bq_gp_predict
 * over the M x n right-hand sides c(q, X).  M == 0 returns BQ_OK and writes nothing.  The call
 * keeps no state with the fit and disturbs none; one read-back.
 * Status rules of bq_gp_predict for the handle.  BQ_ERR_BAD_ARG, all checked before anything is
 * allocated, nothing written: every illegal measure of bq_gp_integral / bq_gp_integral_box; keep ==
 * NULL, a flag that is not 0 or 1, all flags set or none; a covariance that is not symmetric, or
 * whose Sigma_SS, W_I + Sigma_c or W_I + 2 Sigma_c has no Cholesky factor on the host; M < 0, xq
 * == NULL with M > 0, a kept coordinate of xq that is not finite; all three outputs NULL. */
int bq_gp_marginal(bq_ctx *ctx, bq_fit *fit, const int32_t *keep, const double *mu,
                   const double *cov, const double *xq, int64_t M, double *mean, double *var,
                   double *cov_out);
int bq_gp_marginal_box(bq_ctx *ctx, bq_fit *fit, const int32_t *keep, const double *lo,
                       const double *hi, const double *xq, int64_t M, double *mean, double *var,
                       double *cov_out);
/* Square-root-warped Bayesian quadrature of a resident fit (WSABI-L, Gunter et al. 2014) for an
 * integrand l >= alpha0: the fit's targets are g = sqrt(2 (l - alpha0)), one zero-mean GP, and
 * l = alpha0 + g^2 / 2 is linearised about the posterior mean m(x) = k(x, X) alpha, alpha =
 * Kxx^-1 y.  Then l is a GP again with mean alpha0 + m^2 / 2 >= alpha0 and covariance m(x)
 * Sigma(x, x') m(x'), and int l N(. | mu, Sigma) has mean alpha0 + sq / 2 and the variance of
 * Z = int m(x) g(x) N(x | mu, Sigma) dx -- closed form for this kernel, no candidate points and no
 * second GP.  mu, cov as bq_gp_integral takes them.  With Lambda = diag(w^2), Kxx = L L^T,
 *   W(p, q) = int k(p, t) k(t, q) N(t | mu, Sigma) dt
 *           = h^4 N(p - q | 0, 2 Lambda) N((p + q) / 2 | mu, Lambda / 2 + Sigma),
 *   r       = W(X, X) alpha                       (n entries: the kernel means of Z at the fit),
 *   b_w     = L^-1 r,
 *   kappa_i = h^2 N(x_i | mu, Lambda + Sigma),  S = (Lambda^-1 + Sigma^-1)^-1,
 *   Q_ij    = h^2 kappa_i kappa_j N(S Lambda^-1 (x_i - x_j) | 0, Lambda + 2 S)
 *                                                  (bq_int_int_K1_K2_K1 with K1 = K2),
 *   qq      = alpha^T Q alpha                     (the prior variance of Z):
 *   *sq  = alpha . r = int m^2 N: the caller's mean is alpha0 + *sq / 2;
 *   *var = qq - b_w . b_w: latent and NOT clamped at 0, like bq_gp_integral's;
 *   r    = the n kernel means above.
 * Any output may be NULL, but not all three.  The sums over pairs of points run on the device
 * over points transformed once to t1 = x / (sqrt 2 w), t2 = Linv (x - mu) / 2 (Linv^T Linv =
 * (Lambda / 2 + Sigma)^-1), a pair being exp(-|t1(p) - t1(q)|^2 / 2 - |t2(p) + t2(q)|^2 / 2): one
 * thread per row point, the columns in fixed slices that are added in ascending order, no
 * floating-point atomics -- the same inputs give the same bits on every call.  r, b_w, b_w . b_w,
 * qq and sq are kept with the fit for the measure they were computed for: a call with the same
 * (mu, Sigma) computes nothing; a call with another measure recomputes them (two pair sums over
 * n x n, one single-vector forward sweep, three reductions -- enqueued without waiting, one
 * read-back).  Unlike bq_gp_integral's state this one depends on the targets: bq_gp_set_y
 * discards it, as do a refit, an append and a removal.
 * Status rules of bq_gp_predict for the handle; BQ_ERR_BAD_ARG for mu or cov == NULL, all three
 * outputs NULL, a non-finite entry of mu or cov, or a diag(w^2) + Sigma, diag(w^2) + 2 Sigma or
 * diag(w^2) + 2 S that is not positive definite -- all checked before anything is allocated, and
 * nothing is written. */
int bq_gp_sqintegral(bq_ctx *ctx, bq_fit *fit, const double *mu, const double *cov, double *sq,
                     double *var, double *r);
/* The greedy design that minimises the posterior variance of Z of bq_gp_sqintegral: which q of A
 * candidates xc (d x A column-major) to observe so that the variance of the warped integral drops
 * the most, one point at a time.  The recurrence, its kernels and its bits per step are
 * bq_gp_zdesign's; what differs is the linear functional it serves.  Sigma_c is the latent
 * posterior covariance (no s^2) over xc with v_a = L^-1 k(x, xc_a) the rows of the sweep's V;
 * nugget >= 0 in absolute units is an observation's noise (of g); tol >= 0 in multiples of qq, the
 * prior variance of Z.
 * With dc = diag Sigma_c (bq_gp_predict's variance bits), u_a = sum_j W(xc_a, x_j) alpha_j -
 * v_a . b_w = Cov(Z, g(xc_a) | data) and *zvar0 = bq_gp_sqintegral's var, for t = 0 .. q - 1:
 *   eligible  a candidate with dc[a] + nugget > 0 that, when nugget == 0, has not been taken;
 *   score[a] = u_a^2 / (dc[a] + nugget): exactly the drop of var Z when g(xc_a) is observed with
 *             noise nugget and the posterior mean m, about which l is linearised, is held at its
 *             current value -- which is what happens when the observation equals the prediction;
 *   p_t      = the eligible candidate with the largest score, the lowest index among equals; a
 *             NaN score comes first;
 *   gain_t   = score[p_t]; the run ends with rank = t unless gain_t > tol qq, is positive and is
 *             finite;
 *   den      = sqrt(dc[p] + nugget),
 *   c        = (K(xc, xc_p) - V V[p]^T - sum_{i<t} c_i c_i[p]) / den;
 *   u -= c (u_p / den), dc -= c o c (each entry one fma).
 * nugget == 0: c[p] = den, a taken candidate keeps dc = 0 and u = 0 exactly, has c = 0 from then
 * on and is never taken twice.  nugget > 0: a candidate may be taken again and nothing is zeroed.
 * So var Z after t steps is zvar0 - sum_{i<t} gain_i, and with nugget = s^2 that is the var
 * bq_gp_sqintegral returns after bq_gp_append of the chosen points with targets equal to the
 * posterior mean there (other targets move m and with it the functional).  Step 0's scores are the
 * acquisition surface.
 * Outputs on the host: piv (q, -1 from rank on), gain (q, 0 from rank on), zvar0 and rank (one
 * value each) are required; resid_u (A: u after the last step), resid_c (A: dc) and score0 (A:
 * step 0's scores, 0 where a candidate is not eligible) may be NULL.
 * The same inputs give the same bits on every call, and the first j pivots and gains of a q-step
 * call are bit for bit those of a j-step call.
 * Status rules of bq_gp_predict for the handle; BQ_ERR_BAD_ARG as in bq_gp_sqintegral for mu and
 * cov, and for A < 0, q < 1, q > A (but for A == 0), A > BQ_PIVCHOL_MAX_M, q > BQ_PIVCHOL_MAX_Q, a
 * negative or non-finite nugget or tol, or piv, gain, zvar0, rank or -- unless A == 0 -- xc ==
 * NULL: all checked before anything is allocated, and nothing is written.  A == 0 writes
 * rank = 0, piv = -1, gain = 0 and zvar0 and touches nothing else.  Device memory (bq_gp_zdesign's,
 * which this call shares, and Ap (2 d + slices) doubles for the candidates' coordinates and pair
 * sums; kept with the fit) is allocated before anything is enqueued: BQ_ERR_NOMEM leaves the fit as
 * it was.  bq_gp_sqintegral's state for (mu, Sigma) is computed first where it is not there, with
 * its one read-back: qq scales the stop level.  After that all steps are enqueued without waiting
 * for the device; nothing reaches the caller's memory unless every kernel has completed.  The fit
 * is not disturbed, and bq_gp_zdesign's results on it are bit for bit what they were. */
int bq_gp_sqdesign(bq_ctx *ctx, bq_fit *fit, const double *mu, const double *cov, const double *xc,
                   int64_t A, int64_t q, double nugget, double tol, int64_t *piv, double *gain,
                   double *zvar0, double *resid_u, double *resid_c, double *score0, int64_t *rank);

/* One pass "fit + posterior + log-ML" of ONE problem without keeping a fit
 * object: the bordered-Cholesky pipeline.  Host in / host out. */
int bq_fit_predict(bq_ctx *ctx, const double *x, const double *y, int64_t d, int64_t n,
                   double h, const double *w, double s, const double *xo, int64_t M,
                   double *mean, double *var, double *logml);

/* log marginal likelihood on a grid of G hyper-parameter points sharing the
 * data (x, y): h[G], w[G*d] (point g uses w[g*d .. g*d+d-1]), one s.
 * out[G]; a point whose Gram is not positive definite yields -inf
 * (bq.py:542-548).  chunk = problems factored per batched launch (0 = auto).
 * With s == 0 only the distinct w are factored (at h = 1) and every h is derived from
 * chol(h^2 G) = h chol(G). */
int bq_gp_logml_grid(bq_ctx *ctx, const double *x, const double *y, int64_t d, int64_t n,
                     const double *h, const double *w, double s, int64_t G, double *out,
                     int64_t chunk);

/* nprob independent problems of equal size: x[p] is d x n, y[p] has n entries,
 * xo[p] is d x M; all concatenated problem after problem.  Hyper-parameters
 * are shared.  mean/var: nprob x M, logml: nprob, status: nprob (0 ok, >0 the
 * failing column).  This is the unit that shards across GPUs: each rank calls
 * it on its own slice with its own context; there is no collective. */
int bq_batch_fit_predict(bq_ctx *ctx, int64_t nprob, const double *x, const double *y,
                         int64_t d, int64_t n, double h, const double *w, double s,
                         const double *xo, int64_t M, double *mean, double *var, double *logml,
                         int32_t *status);

/* ---- closed-form Gaussian-kernel integrals (gauss_c.pyx) ------------ */
/* Host buffers in and out; points d x n, w / mu length d, cov d x d (symmetric).
 * out_i = h^2 N(x_i | mu, diag(w^2) + cov)                       gauss_c.pyx:95-164 */
int bq_int_K(bq_ctx *ctx, const double *x, int64_t d, int64_t n, double h, const double *w,
             const double *mu, const double *cov, double *out);
/* The same under the uniform measure on the box [lo, hi] and under the mixture (C, pi, mu, cov):
 * out_i = kappa(x_i) and *kk (one double on the host) as bq_gp_integral_box and bq_gp_integral_mix
 * define them.  Either output may be NULL, but not both; kk alone needs no points (n == 0).
 * BQ_ERR_BAD_ARG for the measures as there. */
int bq_int_K_box(bq_ctx *ctx, const double *x, int64_t d, int64_t n, double h, const double *w,
                 const double *lo, const double *hi, double *out, double *kk);
int bq_int_K_mix(bq_ctx *ctx, const double *x, int64_t d, int64_t n, double h, const double *w,
                 int64_t C, const double *pi, const double *mu, const double *cov, double *out,
                 double *kk);
/* The cross matrix and the prior's diagonal of bq_gp_marginal and bq_gp_marginal_box at host
 * points without a fit: out (M x n column-major) = c(xq_i, x_j), pdiag (M) = P(xq_i, xq_i), by the
 * kernels those entry points run.  xq: d x M (integrated axes' rows never read), x: d x n, keep:
 * d flags.  Either output may be NULL, but not both; pdiag alone needs no x (n == 0); M == 0
 * writes nothing.  BQ_ERR_BAD_ARG for h, w, the measure, keep and xq as there. */
int bq_marginal_K(bq_ctx *ctx, const double *xq, int64_t M, const double *x, int64_t n, int64_t d,
                  double h, const double *w, const int32_t *keep, const double *mu,
                  const double *cov, double *out, double *pdiag);
int bq_marginal_K_box(bq_ctx *ctx, const double *xq, int64_t M, const double *x, int64_t n,
                      int64_t d, double h, const double *w, const int32_t *keep, const double *lo,
                      const double *hi, double *out, double *pdiag);
/* out (n1 x n2) = int K1(x1, x') K2(x', x2) N(x' | mu, cov) dx'    gauss_c.pyx:235-339 */
int bq_int_K1_K2(bq_ctx *ctx, const double *x1, int64_t n1, const double *x2, int64_t n2,
                 int64_t d, double h1, const double *w1, double h2, const double *w2,
                 const double *mu, const double *cov, double *out);
/* out (n x n) = int int K1 K2 K1                                   gauss_c.pyx:416-531 */
int bq_int_int_K1_K2_K1(bq_ctx *ctx, const double *x, int64_t d, int64_t n, double h1,
                        const double *w1, double h2, const double *w2, const double *mu,
                        const double *cov, double *out);
/* out (n) = int int K1 K2                                          gauss_c.pyx:617-713 */
int bq_int_int_K1_K2(bq_ctx *ctx, const double *x, int64_t d, int64_t n, double h1,
                     const double *w1, double h2, const double *w2, const double *mu,
                     const double *cov, double *out);

/* ---- BQ moments on device-resident fits (bq_c.pyx) ------------------- */
/* X <- Kxx^-1 B with the resident factor of `fit`; B, X are n x nrhs (host) */
int bq_gp_solve(bq_ctx *ctx, bq_fit *fit, const double *B, int64_t nrhs, double *X);
/* E[Z] = (int K_l(x, x_sc) p(x) dx) . alpha_l, fused on the device: gp_l is the fit
 * of the second GP (its points are x_sc)                           bq_c.pyx:157-213 */
int bq_bq_Z_mean(bq_ctx *ctx, bq_fit *gp_l, const double *mu, const double *cov, double *out);
/* V(Z) = alpha' (int int K_l K_tl K_l) alpha - beta' K_tl^-1 beta, beta =
 * (int K_tl K_l) alpha; nothing n x n is materialised              bq_c.pyx:264-355 */
int bq_bq_Z_var(bq_ctx *ctx, bq_fit *gp_log_l, bq_fit *gp_l, const double *mu, const double *cov,
                double *out);

/* Active-sampling acquisition, batched over M candidate locations x_a (1-D):
 * for each a, the Gram of [x_sc, x_a[a]] (no noise, the reference's jitter on the
 * candidates within `thresh` of x_a[a] and on the new point) is factored and
 * A = K^-1 int K p is reduced to A_a[a] = A[last] and A_sc_l[a] = A[:nsc] . l_sc
 * -- the two numbers bq_c._esm_and_em needs (bq.py:447-527, bq_c.pyx:425-490).
 * One batched bordered Cholesky instead of M sequential refactorisations.
 * status[a] > 0: the system of candidate a is not positive definite. */
int bq_esm_batch(bq_ctx *ctx, const double *x_sc, const double *l_sc, int64_t ns, int64_t nsc,
                 const double *x_a, int64_t M, double h, double w, double thresh, const double *mu,
                 const double *cov, double *A_a, double *A_sc_l, int32_t *status);
/* The same quantities as bq_esm_batch, as a bordered UPDATE of gp_l's resident factor
 * instead of M refactorisations (bq.py:447-527 with the jitter rule of bq_c.pyx:136): one
 * multi-right-hand-side solve for the M borders, the candidate unit vectors, int K p and
 * l_sc, then a c x c Woodbury system per candidate (c = candidates within `thresh`).
 * gp_l: the fit over (x_sc, l_sc), samples first (ns of them), noise-free (s = 0) --
 * BQ_ERR_BAD_ARG otherwise.  status[a] = 1 where the bordered matrix is not positive
 * definite (the reference's LinAlgError fallback, bq.py:481-490). */
int bq_esm_border(bq_ctx *ctx, bq_fit *gp_l, int64_t ns, const double *x_a, int64_t M,
                  double thresh, const double *mu, const double *cov, double *A_a,
                  double *A_sc_l, int32_t *status);

/* ---- resident batch pipeline (what bench.py times) ------------------ */
/* A plan owns device copies of the inputs and all workspaces, so that a run
 * starts with everything resident in HBM and only enqueues kernels. */
/* ---- the stacked pair of GPs at S hyper-parameter sets in one batched pass --------------
 * bq.py:536-550, 933-965 (the hyper-parameter objective) and bq.py:604-662 (marginalize /
 * choose_next over sampled hyper-parameters) evaluate one parameter set after the other; the
 * sets are independent and run here as one batch.  GP1 is the GP over tl_s = log l_s at the
 * samples x_s, GP2 the GP over [l_s, exp(mean of GP1 at x_c)] at [x_s, x_c].  A pair object
 * keeps the points resident for S parameter sets; with ma > 0 acquisition points x_a it serves
 * bq_pair_esm, with ma = 0 bq_pair_llh.  Parameters are S x 3 row-major: (h, w, s) per set. */
typedef struct bq_pair bq_pair;
int bq_pair_create(bq_ctx *ctx, const double *x_s, const double *tl_s, const double *l_s, int64_t ns,
                   const double *x_c, int64_t nc, const double *x_a, int64_t ma, int64_t S,
                   bq_pair **out);
void bq_pair_destroy(bq_ctx *ctx, bq_pair *pair);
/* llh[b] = log_lh(GP1) + log_lh(GP2) under set b, -inf where the reference's closure returns
 * -inf (bq.py:542-548); status[b]: 0 ok, 1 GP1 not positive definite, 2 "GP mean is too large"
 * (bq.py:945-947), 3 GP2 not positive definite.  l_c (S x nc, may be NULL): the candidates'
 * values exp(mean) under every set. */
int bq_pair_llh(bq_ctx *ctx, bq_pair *pair, const double *p_tl, const double *p_l, double *llh,
                double *l_c, int32_t *status);
/* the acquisition's ingredients (bq.py:447-527, bq_c.pyx:425-490) under every set b and for every
 * acquisition point a (element b * ma + a): A_a, A_sc_l with status (1: singular bordered system,
 * the fallback of bq.py:481-490), GP1's posterior mean / variance tm_a, tC_a; per set: l_c (S x nc,
 * may be NULL) and sstatus (1: GP1 not positive definite, 2: GP mean too large). */
int bq_pair_esm(bq_ctx *ctx, bq_pair *pair, const double *p_tl, const double *p_l, double thresh,
                const double *mu, const double *cov, double *A_a, double *A_sc_l, int32_t *status,
                double *tm_a, double *tC_a, double *l_c, int32_t *sstatus);

typedef struct bq_plan bq_plan;
int bq_plan_create(bq_ctx *ctx, int64_t nprob, int64_t d, int64_t n, int64_t M, bq_plan **out);
void bq_plan_destroy(bq_ctx *ctx, bq_plan *plan);
/* upload inputs (host) of all nprob problems; hyper-parameters per problem:
 * h[nprob], w[nprob*d], s[nprob] */
int bq_plan_set_inputs(bq_ctx *ctx, bq_plan *plan, const double *x, const double *y,
                       const double *xo, const double *h, const double *w, const double *s);
/* enqueue one full pass (assemble -> bordered Cholesky -> finalize) */
int bq_plan_run(bq_ctx *ctx, bq_plan *plan);
/* synchronise and copy results out (any pointer may be NULL) */
int bq_plan_results(bq_ctx *ctx, bq_plan *plan, double *mean, double *var, double *logml,
                    int32_t *status);
/* bytes of device memory the plan holds */
int bq_plan_bytes(bq_plan *plan, size_t *bytes);
/* Test aid.  bq_set_guard(1): every device buffer the library allocates from now on carries a
 * 4 KiB sentinel band behind its last byte (also: BQ_GUARD=1 in the environment when the library
 * is loaded).  bq_plan_check_guards synchronises and reports how many of the plan's buffers carry
 * a band and how many sentinel bytes a pass has overwritten (0 for a correct launch sequence).
 * No reference counterpart: the reference's workspaces are numpy arrays (linalg_c.pyx:55-93
 * factors in place); this checks that the batched sweep's block rules size theirs correctly. */
int bq_set_guard(int on);
int bq_plan_check_guards(bq_ctx *ctx, bq_plan *plan, int64_t *guarded, int64_t *damaged);

#ifdef __cplusplus
}
#endif
#endif /* BQHIP_H */
