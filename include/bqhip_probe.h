/*
 * bqhip_probe.h -- hardware probes of libbqhip_probe.so: MFMA / FMA / HBM rates, launch latency,
 * operand layouts, the XCD hand-off study and stamped timelines of the engine's own kernels.
 * They are measurement tools (tools/probe.py, the peak denominators of bench.py --full, the layout
 * and accuracy tests), not part of the product ABI.  libbqhip_probe.so is built from the same
 * objects as libbqhip.so plus the probes, so it also exports every entry point of bqhip.h and a
 * context created by either library is driven by that library's code only (both are linked with
 * -Bsymbolic).
 */
#ifndef BQHIP_PROBE_H
#define BQHIP_PROBE_H

#include "bqhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sustained v_mfma_f64_16x16x4_f64 rate in TFLOP/s over all CUs */
int bq_probe_mfma_f64(bq_ctx *ctx, double *tflops);
/* sustained v_fma_f64 rate in TFLOP/s */
int bq_probe_fma_f64(bq_ctx *ctx, double *tflops);
/* streaming fp64 write / copy bandwidth in GB/s over `bytes` */
int bq_probe_hbm(bq_ctx *ctx, size_t bytes, double *write_gbs, double *copy_gbs);
/* ns per hand-off between two one-wave workgroups (eight ping-pong pairs, the slowest pair):
 * mode 0 = partners on one XCD, plain payload stores + sc1 flag, sc1 loads (no cache maintenance);
 * 1 = partners on different XCDs behind agent-scope release / acquire; 2 = as 1 on one XCD.  kib:
 * KiB of payload per hand-off.  xcc16: the XCC id each of the 16 workgroups ran on; bad_words:
 * payload words that arrived stale.  Bounded spins (status 3 if a partner never answers).
 * Measurement behind docs/LABBOOK.md round 6 (the C2 chain as one launch); no reference
 * counterpart (linalg_c.pyx:55-93 is one LAPACK call). */
int bq_probe_xcd_hop(bq_ctx *ctx, int mode, int64_t iters, int64_t kib, double *ns_per_hop,
                     int32_t *xcc16, int64_t *bad_words);
/* C (m x n) -= P (m x k) Q (n x k)^T on scratch operands through the engine's own kernel
 * selection (lower: only the lower trapezoid; qt: Q given k-contiguous): average ms over `reps`
 * back-to-back launches -- the tuning probe behind tools/gemm_probe.py */
int bq_probe_gemm(bq_ctx *ctx, int64_t m, int64_t n, int64_t k, int lower, int64_t batch, int qt,
                  int64_t reps, double *ms);
/* ONE product C (m x n) -= P (m x k) Q (n x k)^T on the caller's operands, and the route it took.
 * Packed batch elements, column-major: C ldc x n, P ldp x k, Q ldq x k -- or, qt, Q given
 * k-contiguous, Q(j, kk) at Q[j ldq + kk], ldq x n.  lower: only the lower trapezoid is needed;
 * ccut > 0: columns >= ccut need no update; sharing 0 .. 2: how the chip is shared (0 alone, 1 the
 * two streams of a look-ahead, 2 the two halves of a batch); want_fuse: ask for the diagonal
 * factor of C's leading 64 x 64 block in the same launch (failures counted from column j0);
 * seed_d 1 .. 3: a product whose C was left out of the assembly, in seed_d dimensions; rows: a
 * sweep's product (split-k tiles allowed).  C goes up and comes back whole.  route[8], from the
 * launch itself: kernel (0 Lds128, 1 Lds64, 2 Lds64QT, 3 Sub128, 4 Sub64, 5 Sub32, 6 K64x64,
 * 7 K64x32, 8 SplitK), MFMA form of a Sub kernel (4: 4x4x4, 16: 16x16x4, else 0), fused, seeded,
 * assemble_first, grid x / y / z.  When fused: dinv (64 reciprocal pivots per batch element) and
 * info (1-based failing column + j0, or 0, per element).  With C = P = Q = NULL nothing is
 * launched and route[] is the answer for the shape (the only form that takes seed_d > 0).
 * Status 2 for sizes that are not multiples of 16 (k: 8) or anything else out of range. */
int bq_probe_gemm_product(bq_ctx *ctx, double *C, int64_t ldc, const double *P, int64_t ldp,
                          const double *Q, int64_t ldq, int64_t m, int64_t n, int64_t k, int lower,
                          int64_t batch, int qt, int64_t ccut, int sharing, int want_fuse, int64_t j0,
                          int seed_d, int rows, double *dinv, int32_t *info, int32_t *route);
/* `reps` read-only passes over `bytes` with 8-byte-per-lane loads, 512 contiguous bytes per
 * wave (the access pattern of the single-vector sweeps): a known byte count for calibrating
 * the profiler's FETCH_SIZE counter on that pattern; read_gbs may be NULL */
int bq_probe_hbm_read8(bq_ctx *ctx, size_t bytes, int64_t reps, double *read_gbs);
/* MFMA issue study: kind 0 = v_mfma_f64_16x16x4_f64, 1 = v_mfma_f64_4x4x4_4b_f64; nacc
 * independent accumulators per wave (1,2,4,8); blocks_per_cu = waves per SIMD */
int bq_probe_mfma_variant(bq_ctx *ctx, int kind, int nacc, int blocks_per_cu, double *tflops);
/* operand map of v_mfma_f64_4x4x4_4b_f64 under the CBSZ / ABID broadcast controls:
 * out[2*(la*64 + lb) + {0,1}] = low / high half of the 64-bit mask of D lanes fed by A lane la
 * and B lane lb */
int bq_probe_mfma444_layout(bq_ctx *ctx, int cbsz, int abid, int32_t *out8192);
/* out[i] = the Gram kernels' own exp (exp_gauss, csrc/common.h) of x[i] <= 0: per-element
 * accuracy probe (tests/test_gpu_parity.py::test_exp_gauss_accuracy_on_probe_library). */
int bq_probe_exp(bq_ctx *ctx, const double *x, int64_t n, double *out);
/* device time per launch of a chain of n empty, dependent kernels (us) */
int bq_probe_launch(bq_ctx *ctx, int64_t n, double *us_per_launch);
/* One eager pass of a plan (one or two problems, outer block 64) with the profiling
 * instantiation of the one-launch slab step: 160 s_memtime stamps of workgroup 0 per step
 * (10 phase boundaries, then the diagonal factor's per-wave barrier stamps). */
int bq_probe_c2_timeline(bq_ctx *ctx, bq_plan *plan, int64_t *stamps, int64_t nsteps);
/* The first launch of a small system's sweep alone -- the assembly with the leading block's factor
 * folded in (csrc/slab.h, assemble_first_kernel; BQ_FIRST_REGS selects its form) -- on `batch`
 * problems of n points in d dimensions with M prediction points (x: batch x n x d, y: batch x n,
 * xo: batch x M x d; one h, w[d], s for all), and what it leaves in memory, every buffer preset to
 * 0xA5 bytes: Acol, the first 64 columns of every system (batch x 64 x ntot, column-major, ld
 * ntot: the leading block's strict upper triangle, its factor, the unsolved rows below); S0, the
 * sweep's scratch column (batch x 64 x ntot); dinv (batch x BQ_DINV_STRIDE doubles); info (batch);
 * scal (batch x 4).  ntot = roundup(roundup(n, 64) + M + 1, 64) and dinv_len = the record's doubles as
 * the caller sized its buffers for them: anything else is BQ_ERR_BAD_ARG.  stamps16 (null, or d = 1): 16
 * s_memtime values of workgroup (0, 0) of problem 0 -- entry, block assembled, then the factor's
 * five phase boundaries.  (tests/test_first_launch.py) */
int bq_probe_first_launch(bq_ctx *ctx, int64_t batch, int64_t d, int64_t n, int64_t M,
                          const double *x, const double *y, const double *xo, double h,
                          const double *w, double s, int64_t ntot, int64_t dinv_len, double *Acol,
                          double *S0, double *dinv, int32_t *info, double *scal, int64_t *stamps16);
/* The 64 x 64 diagonal factor alone (the launch that heads every panel step): A is a
 * 64 x 64 host matrix, factored `reps` times from a resident copy (from_lds != 0: handed
 * over through LDS as the one-launch steps do).  Last launch's factor, its
 * BQ_DINV_HALF-double record (64 reciprocal pivots + four 16 x 16 block inverses), info,
 * HIP-event microseconds per launch and 136 in-kernel s_memtime stamps (5 phase
 * boundaries, then per panel and wave the arrival at / release from the panel barrier).
 * from_lds bit 0: through LDS; bit 1: eight waves; bit 2: per-wave stamps; bits 8-14: nreal, the
 * block's real columns when fewer than 64 (A is then identity from row / column nreal on: the
 * padded steps and their epilogue); 0 = a full block. */
int bq_probe_potf2(bq_ctx *ctx, const double *A, int from_lds, int64_t reps, double *L_out,
                   double *dinv_out, int32_t *info_out, double *us_per_launch,
                   int64_t *stamps136);
/* Both producers of the block-inverse records on one factor: A (128 x 128, host, column-major,
 * ld 128, in: SPD, out: its factor by the one-launch steps), rec_sweep: the two records the steps
 * left in the ping-pong halves (2 x BQ_DINV_HALF doubles: block 0, block 1), rec_resident: the
 * records diag_winv_kernel builds from the factor in memory, as for a resident fit (the same
 * layout).  BQ_ERR_BAD_ARG when the context would not run the one-launch steps.
 * (tests/test_block_inverse.py) */
int bq_probe_records(bq_ctx *ctx, double *A, double *rec_sweep, double *rec_resident,
                     int32_t *info);
/* The batched panel solve of one outer block alone (potrf.hip, enqueue_panel_solve): X (m x kb per
 * problem, column-major, in / out) <- X L^-T against `batch` dense lower-triangular kb x kb
 * factors L; mode 0: as the context is configured, 1: recursive products + 64-column solves,
 * 2: the one-launch sweep (trsm_sweep_kernel); any other mode is BQ_ERR_BAD_ARG.  m, kb multiples
 * of 64.  reps > 0: the call is
 * repeated reps times on its own output and timed (HIP events, ms per call); X is then not
 * written back. */
int bq_probe_panel_solve(bq_ctx *ctx, int64_t m, int64_t kb, int64_t batch, const double *L,
                         double *X, int mode, int64_t reps, double *ms_per_call);
/* The batched Cholesky sweep on the caller's own matrices (potrf.hip, enqueue_potrf_partial; a plan
 * takes points, so nothing else can hand a batched route a dense or a deliberately indefinite
 * matrix): the first ncols columns of `batch` lower ntot x ntot matrices (column-major, leading
 * dimension lda, astride doubles apart; 0 = the plans' own padded lda / lda * ntot) are
 * eliminated along the route the engine picks for (ntot, ncols, batch), with its workspace sized
 * as a plan's and nothing seeded or skipped: L11 and L21 replace the first ncols columns, the
 * lower triangle of the Schur complement the rest.  A (host, batch * astride doubles) is uploaded
 * and downloaded whole -- rows ntot .. lda - 1 and the gaps between matrices must come back as
 * they went.  info[b]: 0 or the 1-based failing column of matrix b.  route[0..2]: the sweep that
 * ran (0 one-launch steps, 1 blocked, 2 two half-batches, 3 diagonal block first), its outer
 * block, and whether it used scratch.  ntot, ncols multiples of 64, ncols <= ntot, lda >= ntot and
 * even, astride >= lda * ntot and even; anything else is BQ_ERR_BAD_ARG.
 * (tests/test_cholesky_contracts.py) */
int bq_probe_potrf_batch(bq_ctx *ctx, int64_t batch, int64_t ntot, int64_t ncols, int64_t lda,
                         int64_t astride, double *A, int32_t *info, int32_t *route);
/* ONE triangular sweep over a resident factor on the caller's own factor and right-hand sides
 * (csrc/sweeps.hip; bq_cho_solve always runs a forward and a backward sweep, a fit takes points).
 * L: n x n lower factor (host, column-major, ld n), uploaded with leading dimension ldl (0: the
 * engine's own; >= n, may be odd); the 16 x 16 and the wide block inverses are built from it as
 * bq_cho_solve builds them.  X: the right-hand sides as ROWS, X[r + j ldx], mrows x n, in and out;
 * the whole ldx x n buffer is uploaded and downloaded, rows mrows .. ldx - 1 must come back as they
 * went.  which:
 *   BQ_SWEEP_FORWARD_ROWS       X <- X L^-T (enqueue_forward_rows)
 *   BQ_SWEEP_BACKWARD_ROWS      X <- X L^-1 (enqueue_backward_rows)
 *   BQ_SWEEP_FORWARD_ROWS_BLK   X <- X L^-T in 64-column steps from the 16 x 16 inverses
 *   BQ_SWEEP_INVERSE_ROWS       X <- L^-T, its strict lower triangle zero (X ignored on input;
 *                               mrows = ldx = n)
 *   BQ_SWEEP_FORWARD_VEC / BQ_SWEEP_BACKWARD_VEC             one vector (mrows = 1: X[j ldx]),
 *                               x <- L^-1 x / L^-T x, one launch per block column
 *   BQ_SWEEP_FORWARD_VEC_FLOW / BQ_SWEEP_BACKWARD_VEC_FLOW   the same as one launch, with
 *                               bq_cho_solve's fall-back; BQ_ERR_BAD_ARG where the engine has no
 *                               one-launch sweep for n
 * route[0..4]: the kind that ran (BQ_SWEEP_KIND_*), the columns per step, the fused steps whose
 * update went out as LDS-staged tiles and as split-k tiles, and the context's count of one-launch
 * sweeps re-issued after a timed-out hand-off.  n a multiple of 64, mrows a multiple of 32 (1 for
 * the single-vector sweeps), ldx >= mrows, ldl >= n; anything else is BQ_ERR_BAD_ARG.
 * (tests/test_sweep_contracts.py) */
enum {
    BQ_SWEEP_FORWARD_ROWS = 0,
    BQ_SWEEP_BACKWARD_ROWS = 1,
    BQ_SWEEP_FORWARD_ROWS_BLK = 2,
    BQ_SWEEP_INVERSE_ROWS = 3,
    BQ_SWEEP_FORWARD_VEC = 4,
    BQ_SWEEP_BACKWARD_VEC = 5,
    BQ_SWEEP_FORWARD_VEC_FLOW = 6,
    BQ_SWEEP_BACKWARD_VEC_FLOW = 7
};
enum {
    BQ_SWEEP_KIND_STEP = 0,      /* one split-k launch per block (small systems, forward) */
    BQ_SWEEP_KIND_FUSED = 1,     /* one launch per block, solve and update side by side */
    BQ_SWEEP_KIND_GEMM_ROWS = 2, /* two products per block */
    BQ_SWEEP_KIND_BLK = 3,
    BQ_SWEEP_KIND_VEC_BLOCK = 4,
    BQ_SWEEP_KIND_VEC_FLOW = 5
};
int bq_probe_sweep(bq_ctx *ctx, int which, int64_t n, const double *L, int64_t ldl, int64_t mrows,
                   int64_t ldx, double *X, int32_t *route);
/* dump of the f64 MFMA D-register layout: out[64*4] receives, for lane l and
 * register r, the value row*16+col of the D element it holds */
int bq_probe_mfma_layout(bq_ctx *ctx, double *out256);

#ifdef __cplusplus
}
#endif
#endif /* BQHIP_PROBE_H */
