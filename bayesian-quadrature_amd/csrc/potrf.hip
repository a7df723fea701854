// potrf.hip -- the launch sequences of the blocked right-looking Cholesky: block sizes and the
// route of a sweep (sweep_route), recursive panels, the one-launch sweeps of small systems, the
// two-stream look-ahead, two half-batches, diagonal block first, and the bordered pass of plans
// and fits.  No kernels of its own (k_panel.hip, k_gemm.hip).
#include "host.h"

namespace bqh {

// A batch's diagonal factors (enqueue_potrf_dfirst): one workgroup per matrix from 96 matrices on
// -- the workgroups then cover the chip, and unlike the one-launch steps they solve nothing
// twice --, the one-launch steps below (64 matrices would leave three quarters of the CUs without
// a factor to work on: 366 us alone against 236).  BQ_DF_WG = 0 / 1 forces either.
static bool dfirst_wg(const bq_ctx *c, int batch) { return c->cfg.df_wg < 0 ? batch >= 96 : c->cfg.df_wg != 0; }

// One or two matrices below kSlabNbMax rows run the one-launch steps throughout (auto_nb); the last
// kSlabMax rows of a larger one are handed to them (enqueue_potrf_group)
constexpr int kSlabNbMax = 3072;
constexpr int kSlabMax = 4800;

int auto_nb(const bq_ctx *c, int ntot, int batch)
{
    if (c->cfg.nb_override > 0)
        return c->cfg.nb_override;
    // the trailing update re-reads and re-writes the whole remaining matrix once per
    // outer block: when the batch's matrices do not fit the caches the outer block
    // must be wide (256: 46 GB instead of 183 GB of traffic at N=16384), when they do
    // a narrow block means fewer, shorter launches
    const double mb = 8.0 * (double)ntot * ntot * batch / 1e6;
    if (batch <= 2) {
        // One or two matrices cannot fill the chip with a 64-column panel: the sweep is a
        // chain of dependent launches and the one-launch step of outer block 64 (slab.h) is
        // the shortest chain until the k = 64 updates cost more than it saves.  Re-measured in
        // round 3 with the 64-tile trailing updates (tools/potrf_sizes.py on one matrix, ms with
        // blocks 64 / 256: N=2560 0.761 / 0.774, 3072 1.013 / 0.995, 3584 1.346 / 1.318, 4096
        // 1.776 / 1.617, 4608 2.311 / 1.967): from 3072 rows the first panels are blocked (with
        // the look-ahead once there is room for it) and the LAST rows go to the one-launch steps
        // (kSlabMax / la_min, enqueue_potrf_group)
        if (ntot < kSlabNbMax)
            return 64;
        // a wider block halves the trailing update's C traffic per flop (60 instead of 56
        // TFLOP/s at k = 512); it pays once the panel it lengthens hides behind the bulk
        // update (round 3, ms with 256 / 320 / 384 / 512: N = 5120 2.354 / 2.330 / 2.289 / 2.378,
        // 8192 5.432 / 5.357 / 5.306 / 5.416, 10240 8.687 / 8.552 / 8.441 / 8.422, 12288 13.29 /
        // 12.92 / 12.79 / 12.71, 16384 27.36 / 26.72 / 26.19 / 26.00)
        return ntot < 9216 ? 384 : 512;
    }
    // A few small matrices (the stacked parameter sets of the hyper-parameter loops: 5-6 systems
    // of the sample count) are a chain of dependent launches like one matrix is, and the
    // one-launch steps stay the shortest chain while a step's workgroups -- batch x T (T + 1) / 2
    // tiles, each with its redundant panel solves -- fit the chip about five times over
    // (tools/nb_sweep.py, ms with blocks 64 / 128 / 256: 5 x N=1024 0.377 / 0.475 / 0.512,
    // 12 x 1024 0.564 / 0.611 / 0.664, 16 x 1024 0.667 / 0.648 / 0.697, 8 x 1536 0.940 / 0.953 /
    // 0.977, 5 x 2048 1.237 / 1.138 / 1.185; the hyper-parameter objective + gradient at 1024
    // samples 0.99 -> 0.78 ms)
    const long T = ntot / 64;
    if ((long)batch * T * (T + 1) / 2 <= 2500)
        return 64;
    // (batches of mid-sized matrices, recursive panels: C5 shard 6.55 / 6.42 / 6.70 / 6.57 ms
    // with 256 / 320 / 384 / 512; 256 x C2 5.72 / 5.47 / 5.64 ms with 256 / 320 / 448; below
    // half a gigabyte 128 is still ahead: 12 x N=2048 1.694 / 1.716, 16 x 2048 2.024 / 1.954,
    // 5 x 3072 2.250 / 2.272, 8 x 3072 3.069 / 2.856 with 128 / 256)
    // (re-measured at the end of round 3, 320 against 448 in one box: C3 190.4 / 187.0 ms,
    // 256 x C2 5.23 / 5.16, C5 shard 5.82 / 5.80)
    // (round 4, diagonal block first, ms with 320 / 384 / 448 / 512 in one box: C5 shard 5.85 / 5.78 /
    // 5.71 / 5.90 on the one-launch steps; with a workgroup per matrix 256 x C2 4.45 / 4.32 / 4.50 /
    // 4.52, the C3 grid 188 / 178 / 190 / 180)
    if (ntot >= 1024 && mb >= 500.0)
        return (c->cfg.diag_first && dfirst_wg(c, batch)) ? 384 : 448;
    if (ntot >= 512)
        return 128;
    return 64;
}

// doubles of scratch the one-launch slab sweep needs (two panel columns per problem)
static size_t panel_ws_doubles(int ntot, int batch) { return ((size_t)2 * 64 * ntot + 4096) * batch; }
// the block-inverse records of one outer block's diagonal factor (enqueue_potrf_dfirst)
static size_t dfirst_rec_doubles(int nb, int batch) { return (size_t)(nb / 64) * BQ_DINV_HALF * batch; }

// the look-ahead pays up to this many matrices per batch (enqueue_potrf_group)
#define BQ_LA_MAX_BATCH 48

SweepRoute sweep_route(const bq_ctx *c, int ntot, int ncols, int batch, size_t ws_on_hand)
{
    SweepRoute r{};
    r.ntot = ntot;
    r.ncols = ncols;
    r.batch = batch;
    r.nb = auto_nb(c, ntot, batch);
    // A blocked sweep (outer block >= 128) reads a bordered system's results off the border rows
    // and skips the border x border block in its trailing updates; the one-launch steps of small
    // systems update everything and read the Schur complement.
    r.border_rows = r.nb >= 128;
    if (c->cfg.diag_first && batch >= 3 && ncols >= 128 && r.nb >= 128) {
        // (two sets of records: with the early fork the next block's diagonal factor writes its own
        // while the rest of this block's panel solve still reads this block's)
        const int nb = std::min(r.nb, ncols);
        const size_t need = panel_ws_doubles(nb, batch) + 2 * dfirst_rec_doubles(nb, batch);
        if (ws_on_hand >= need) {
            r.kind = SweepRoute::DiagFirst;
            r.ws_doubles = need;
            // (with one outer block there is no product that could seed what lies right of it)
            r.seed_cols = c->cfg.asm_fuse && nb < ncols ? nb : 0;
            return r;
        }
    }
    const size_t panel = panel_ws_doubles(ntot, batch);
    if (r.nb == 64 && ncols >= 64 && ws_on_hand >= panel) {
        r.kind = SweepRoute::Slab;
        r.ws_doubles = panel;
        r.first_in_assembly = ntot > 64;
        return r;
    }
    // large systems (a look-ahead's size) in a batch that fills the chip many times over run
    // as ONE sequential group: the product is power-bound (docs/LABBOOK.md section 4), beside it the
    // panel chain only takes clock away (C3, 100 x N = 4096: 189.8 ms with the look-ahead,
    // 198 in two halves, 186.3 sequential; up to 32 matrices the look-ahead still gains 1-2 %)
    const bool big = ncols > r.nb && ntot - std::min(r.nb, ncols) >= c->cfg.la_min;
    if (c->cfg.lookahead && c->aux && c->cur == c->stream && batch >= 8 && r.nb >= 128 && !big) {
        r.kind = SweepRoute::Halves;
        return r;
    }
    r.kind = SweepRoute::Blocked;
    // (a batch fills the chip without the panel steps and the slab tail: only one or two
    // matrices use the scratch)
    if (batch <= 2 && ws_on_hand >= panel)
        r.ws_doubles = panel;
    return r;
}

// The trailing update of block (r_row, r_col) by the panel that starts at column K0:
// A[r_row.., r_col..] (m x n) -= A[r_row.., K0..] A[r_col.., K0..]^T over k columns
static GemmJob trailing_job(double *A, long lda, long astride, int r_row, int r_col, int K0, int m,
                            int n, int k, int lower, int batch)
{
    GemmJob g;
    g.C = A + r_row + (long)r_col * lda, g.ldc = lda, g.cstride = astride;
    g.P = A + r_row + (long)K0 * lda, g.ldp = lda, g.pstride = astride;
    g.Q = A + r_col + (long)K0 * lda, g.qsj = 1, g.qsk = lda, g.qstride = astride;
    g.m = m, g.n = n, g.k = k;
    g.lower = lower, g.batch = batch;
    return g;
}

// Columns [j0, j0 + w) of a panel, recursively: the left half, ONE update of the right half's
// columns with the whole left half, the right half.  Same flops as the left-looking slab
// order (each 64-column slab updated with everything before it, n = 64 per launch), but two
// thirds of a 256-wide panel's update flops are then ONE n = 128, k = 128 product -- wide
// enough for the LDS-staged kernel -- instead of two n = 64 launches that re-stream the panel
// (a batch's panel does not fit in L2: the n = 64 updates ran at 12 TFLOP/s; C5 shard
// 6.8 -> see DESIGN).  A 64-column slab: its diagonal factor (unless the launch that last
// updated it carried it, GemmRoute::fused: diag_done) and the solve of the rows below.
static int enqueue_panel_rec(bq_ctx *c, double *A, long lda, long astride, int batch, int ntot, int j0,
                      int w, double *dinv, int *info, bool diag_done)
{
    if (w <= 64) {
        double *Ajj = A + j0 + (long)j0 * lda;
        if (!diag_done)
            BQCHK(launch_potf2(c, A, lda, astride, j0, dinv, BQ_DINV_STRIDE, info, batch));
        return launch_trsm_blk(c, Ajj + 64, lda, astride, ntot - j0 - 64, Ajj, lda, astride, dinv,
                               BQ_DINV_STRIDE, batch);
    }
    const int wl = ((w / 64 + 1) / 2) * 64, wr = w - wl;
    BQCHK(enqueue_panel_rec(c, A, lda, astride, batch, ntot, j0, wl, dinv, info, diag_done));
    const int r0 = j0 + wl;
    GemmJob g = trailing_job(A, lda, astride, r0, r0, j0, ntot - r0, wr, wl, 1, batch);
    g.fuse = {r0, dinv, BQ_DINV_STRIDE, info};
    GemmRoute ran;
    BQCHK(launch_gemm(c, BQ_K_GEMM, g, &ran));
    return enqueue_panel_rec(c, A, lda, astride, batch, ntot, r0, wr, dinv, info, ran.fused);
}

// the 64-column slabs of one outer block [K0, K0+KB): left-looking update, diagonal
// factor, panel solve -- enqueued on c->cur.  With fusion on, the diagonal factor of a
// slab rides in the launch that last updates it (the slab update here, or the
// trailing update of the previous block: `diag_done`).
// With a scratch column pair `ws` (panel_ws_doubles; one or two matrices) every step is ONE
// launch (panel_step_kernel, slab.h): the workgroups solve the rows they need themselves.
static int enqueue_panel(bq_ctx *c, double *A, long lda, long astride, int batch, int ntot, int K0,
                  int KB, double *dinv, int *info, bool diag_done, double *ws = nullptr)
{
    if (ws) {
        if (!diag_done)
            BQCHK(launch_potf2(c, A, lda, astride, K0, dinv, BQ_DINV_STRIDE, info, batch));
        if (ntot - K0 - 64 <= 0)
            return BQ_OK;
        const long sstride = 64L * ntot;
        double *S[2] = {ws, ws + sstride * batch};
        double *SL = ws + 2 * sstride * batch; // 64 x 64 per problem
        const int ns = KB / 64;
        for (int sidx = 0; sidx < ns; ++sidx) {
            const int j0 = K0 + 64 * sidx;
            const int nrb = (ntot - j0 - 64) / 64;
            if (nrb <= 0)
                break;
            const int has_next = sidx + 1 < ns;
            const double m = 64.0 * nrb;
            const int par = sidx & 1;
            BQCHK(launch_panel_step(
                c, A, lda, astride, batch, nrb, S[par], S[par ^ 1], (long)ntot, sstride, K0, j0,
                dinv + par * BQ_DINV_HALF, dinv + (par ^ 1) * BQ_DINV_HALF, has_next, sidx == 0, SL,
                info,
                (m * 64.0 * 64.0 + (has_next ? 2.0 * m * 64.0 * 64.0 * (sidx + 1) : 0.0)) * batch));
        }
        return BQ_OK;
    }
    return enqueue_panel_rec(c, A, lda, astride, batch, ntot, K0, KB, dinv, info, diag_done);
}

// Outer block 64 (small systems): one launch per 64-column step (slab.h) after the first
// diagonal factor and the staging of panel 0.  a: the route's read-out, step 0 in the assembly
// and the probe's stamps (SweepRoute::Slab; the sweeps inside other routes pass none).
// col0: global column of A's first column (a sweep over the trailing block of a larger
// factorisation reports failures in the larger matrix's numbering)
// rstride > 0: `dinv` is a row of RECORDS per problem (rstride doubles apart), one BQ_DINV_HALF
// per 64-column step, and every step's reciprocal pivots / block inverses stay behind in the
// record of its own diagonal block (the batched panel solve reads them: enqueue_potrf_dfirst);
// else the two halves of a BQ_DINV_STRIDE ping-pong.
static int enqueue_slab_sweep(bq_ctx *c, double *A, long lda, long astride, int batch, int ntot,
                       int ncols, double *dinv, int *info, double *ws, const SweepArgs &a,
                       int col0 = 0, long rstride = 0)
{
    const long dstride = rstride > 0 ? rstride : (long)BQ_DINV_STRIDE;
    if (ntot <= 64)
        return launch_potf2(c, A - col0 - (long)col0 * lda, lda, astride, col0, dinv, dstride,
                            info, batch);
    const long sstride = 64L * ntot;
    double *S[2] = {ws, ws + sstride * batch};
    if (!a.first_done)
        // the first diagonal factor and the staging of panel 0 share a launch (or ride in the
        // assembly: assemble_first_kernel)
        BQCHK(launch_slab_first(c, A, lda, astride, batch, S[0], (long)ntot, sstride, ntot, dinv,
                                info, col0, dstride));
    for (int j0 = 0, par = 0; j0 < ncols; j0 += 64, par ^= 1) {
        const int r0 = j0 + 64;
        if (r0 >= ntot)
            break;
        const int fnext = r0 < ncols;
        const double m = (double)(ntot - r0);
        // only batch element 0 is stamped, and only while the probe's buffer has room
        long long *stamps =
            (a.stamps && j0 / 64 < a.stamped_steps) ? a.stamps + 160 * (j0 / 64) : nullptr;
        // the tile updates (lower half of 2 m^2 64) and the solve of the panel (m 64^2)
        const long din = rstride > 0 ? (long)(j0 / 64) * BQ_DINV_HALF : (long)par * BQ_DINV_HALF;
        const long dout =
            rstride > 0 ? (long)(j0 / 64 + 1) * BQ_DINV_HALF : (long)(par ^ 1) * BQ_DINV_HALF;
        BQCHK(launch_slab_step(c, A, lda, astride, batch, S[par], S[par ^ 1], (long)ntot, sstride,
                               ntot, j0, dinv + din, dinv + dout, fnext, !fnext, info, col0, a.out,
                               stamps, (m * m * 64.0 + m * 64.0 * 64.0) * batch, dstride));
    }
    return BQ_OK;
}

// Eliminate the first ncols columns (multiple of 64) of the ntot x ntot lower
// matrix (ntot multiple of 64), batched, with outer block NB.  dinv: BQ_DINV_STRIDE doubles per
// problem.  ws: the slab sweep's scratch (SweepRoute::Blocked of one or two matrices, else null):
// one-launch panel steps and the last rows on the one-launch steps.
//
// With more than one outer block and a wide block the factorisation runs with a
// look-ahead of one panel on two streams.  The main stream carries only the bulk
// trailing updates (everything right of the next panel), back to back; the
// high-priority aux stream updates the next panel's columns and factors that
// panel meanwhile.  The two meet through events: update k+1 waits for panel k+1,
// the panel-column update k+1 waits for trailing update k (which last wrote
// those columns).
// skip_border: the caller reads its results off the border ROWS (plan_readout_kernel), so the
// trailing updates leave the border x border block alone
static int enqueue_potrf_group(bq_ctx *c, double *A, long lda, long astride, int batch, int ntot,
                        int ncols, double *dinv, int *info, double *ws, int NB, bool skip_border)
{
    const bool la = c->cfg.lookahead && c->aux && NB >= 128 && ncols > NB && batch <= BQ_LA_MAX_BATCH;
    int K0 = 0;
    bool panel_done = false; // panel K0 was already factored by the look-ahead phase
    if (la && ntot - std::min(NB, ncols) >= c->cfg.la_min) {
        // fork: the aux stream starts after everything already queued on the main stream
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_fork, 0));
        // aux stream: panel 0
        {
            OnStream aux(c, c->aux);
            BQCHK(enqueue_panel(c, A, lda, astride, batch, ntot, 0, std::min(NB, ncols), dinv, info,
                                false, ws));
        }
        HIPCHK(c, hipEventRecord(c->ev_panel, c->aux));
        bool have_b = false; // a trailing update is in flight on the main stream
        Sharing la_scope(c, 1);
        for (; K0 < ncols; K0 += NB) {
            const int KB = std::min(NB, ncols - K0);
            const int r0 = K0 + KB;
            // main stream: wait for panel K0
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_panel, 0));
            panel_done = true;
            if (r0 >= ntot) {
                K0 = ncols;
                break;
            }
            // Once the bulk update is shorter than the panel chain it has to hide, the two
            // streams only slow each other down (N = 4096: 2.50 ms with, 2.26 ms without):
            // the rest of the sweep runs sequentially on the main stream.
            if (ntot - r0 < c->cfg.la_min)
                break;
            const int nw = (r0 < ncols) ? std::min(NB, ncols - r0) : 0; // width of the next panel
            if (nw > 0) {
                // aux stream: bring the next panel's columns up to date (they were last
                // written by the previous trailing update on the main stream), factor it
                if (have_b)
                    HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_next, 0));
                {
                    OnStream aux(c, c->aux);
                    // (a wide panel's update is worth the LDS-staged kernel, which carries no
                    // fused diagonal factor: enqueue_panel then factors the block itself)
                    GemmJob g = trailing_job(A, lda, astride, r0, r0, K0, ntot - r0, nw, KB, 1, batch);
                    g.fuse = {r0, dinv, BQ_DINV_STRIDE, info};
                    GemmRoute ran;
                    BQCHK(launch_gemm(c, BQ_K_SYRK, g, &ran));
                    BQCHK(enqueue_panel(c, A, lda, astride, batch, ntot, r0, nw, dinv, info,
                                        ran.fused, ws));
                }
                HIPCHK(c, hipEventRecord(c->ev_panel, c->aux));
                // main stream: everything right of the next panel, concurrently
                const int r1 = r0 + nw;
                if (r1 < ntot) {
                    GemmJob b = trailing_job(A, lda, astride, r1, r1, K0, ntot - r1, ntot - r1, KB,
                                             1, batch);
                    b.ccut = skip_border ? ncols - r1 : 0;
                    BQCHK(launch_gemm(c, BQ_K_SYRK, b));
                    HIPCHK(c, hipEventRecord(c->ev_next, c->stream));
                    have_b = true;
                }
            } else {
                // no further panel: the remaining trailing block is pure Schur complement
                BQCHK(launch_gemm(c, BQ_K_SYRK, trailing_job(A, lda, astride, r0, r0, K0, ntot - r0,
                                                             ntot - r0, KB, 1, batch)));
            }
            panel_done = false;
        }
    }
    // sequential sweep: everything without look-ahead, otherwise the rest
    bool diag_done = false;
    for (; K0 < ncols; K0 += NB) {
        const int KB = std::min(NB, ncols - K0);
        if (!panel_done)
            BQCHK(enqueue_panel(c, A, lda, astride, batch, ntot, K0, KB, dinv, info, diag_done,
                                ws));
        panel_done = false;
        const int r0 = K0 + KB;
        diag_done = false;
        // The last rows of a large matrix are a small factorisation of their own -- the
        // Schur complement once this block's update is in --, and for one or two matrices
        // the one-launch steps are its shortest chain: hand the rest to the slab sweep.
        const bool to_slab = ws && NB > 64 && r0 < ncols && ntot - r0 < kSlabMax;
        if (r0 < ntot) {
            GemmJob g = trailing_job(A, lda, astride, r0, r0, K0, ntot - r0, ntot - r0, KB, 1, batch);
            g.ccut = skip_border ? ncols - r0 : 0;
            // the trailing update also factors the next diagonal block if there is one
            if (r0 < ncols && !to_slab)
                g.fuse = {r0, dinv, BQ_DINV_STRIDE, info};
            GemmRoute ran;
            BQCHK(launch_gemm(c, BQ_K_SYRK, g, &ran));
            diag_done = ran.fused;
        }
        if (to_slab)
            return enqueue_slab_sweep(c, A + r0 + (long)r0 * lda, lda, astride, batch, ntot - r0,
                                      ncols - r0, dinv, info, ws, SweepArgs(), r0);
    }
    return BQ_OK;
}

// ---------------------------------------------------------------------------------------------
// Batches, diagonal block first (round 4).  The recursive panels above factor an outer block's
// m x NB panel as a chain of 64-column steps over ALL its rows: per step a one-workgroup diagonal
// factor, a panel solve and a product, each a pass over rows that do not fit a cache (a C5
// shard's panels: 440 MB) -- a third of a batch's sweep at a fifth of the chip's rate, and
// a chain that two half-batches on two streams only hide by slowing each other down.  But
// the rows below an outer block's NB x NB diagonal block take no part in factoring it:
//     D  the diagonal block alone: a small Cholesky (one-launch steps, slab.h), a few MB per
//        matrix, whose 64-column steps leave their block inverses behind in records;
//     S  L21 = A21 L11^-T for all rows below in ONE sweep of throughput launches, recursively
//        (left half, product, right half) with the solve of a product's first 64 columns fused
//        into the product (gemm_trsm64_kernel): NB / 64 launches, none latency-bound;
//     U  the trailing update, k = NB -- first, on the second stream, the NEXT diagonal block
//        and its factorisation D, hidden beside the rest of the update.
// The whole batch moves in lock-step through launches that each fill the chip.
// ---------------------------------------------------------------------------------------------
// X = rows [rx, rx + m) of the panel that starts at column K0: columns [j0, j0 + w) (relative
// to K0) solved against L11 = A[K0.., K0..]; rec: the records of L11's 64 x 64 diagonal blocks.
// solved: the launch that last updated slab j0 solved it as well.
static int enqueue_trsm_rec(bq_ctx *c, double *A, long lda, long astride, int batch, int rx, int m,
                            int K0, int j0, int w, const double *rec, long rstride, bool solved)
{
    if (w <= 64) {
        if (solved)
            return BQ_OK;
        const long cj = K0 + j0;
        return launch_trsm_blk(c, A + rx + cj * lda, lda, astride, m, A + cj + cj * lda, lda,
                               astride, rec + (long)(j0 / 64) * BQ_DINV_HALF, rstride, batch);
    }
    const int wl = ((w / 64 + 1) / 2) * 64, wr = w - wl;
    BQCHK(enqueue_trsm_rec(c, A, lda, astride, batch, rx, m, K0, j0, wl, rec, rstride, solved));
    const long cl = K0 + j0, cr = cl + wl;
    const bool fuse = gemm_trsm_ok(c, m, wr, wl);
    if (fuse)
        // (Q = L11[j0 + wl .., j0 ..): wr x wl)
        BQCHK(launch_gemm_trsm(c, A + rx + cr * lda, lda, astride, A + rx + cl * lda, lda, astride,
                               A + cr + cl * lda, lda, astride, m, wr, wl, A + cr + cr * lda, lda,
                               astride, rec + (long)((j0 + wl) / 64) * BQ_DINV_HALF, rstride, batch));
    else
        BQCHK(launch_gemm(c, BQ_K_GEMM,
                          trailing_job(A, lda, astride, rx, (int)cr, (int)cl, m, wr, wl, 0, batch)));
    return enqueue_trsm_rec(c, A, lda, astride, batch, rx, m, K0, j0 + wl, wr, rec, rstride, fuse);
}

// the panel solve of one outer block as enqueue_potrf_dfirst issues it (also bq_probe_panel_solve);
// one_launch: trsm_sweep_kernel (c->cfg.df_sweep), else the recursive products and solves
int enqueue_panel_solve(bq_ctx *c, double *A, long lda, long astride, int batch, int r0, int m2,
                        int K0, int KB, const double *rec, long rstride, bool one_launch)
{
    if (one_launch)
        return launch_trsm_sweep(c, A + r0 + (long)K0 * lda, lda, astride, m2,
                                 A + K0 + (long)K0 * lda, lda, astride, rec, rstride, KB, batch);
    return enqueue_trsm_rec(c, A, lda, astride, batch, r0, m2, K0, 0, KB, rec, rstride, false);
}

static int enqueue_potrf_dfirst(bq_ctx *c, const SweepRoute &r, double *A, long lda, long astride,
                                int *info, double *ws, const SweepArgs &a)
{
    const int batch = r.batch, ntot = r.ntot, ncols = r.ncols, NB = std::min(r.nb, ncols);
    const bool skip_border = a.skip_border, one_launch = c->cfg.df_sweep;
    double *recs[2] = {ws + panel_ws_doubles(NB, batch),
                       ws + panel_ws_doubles(NB, batch) + dfirst_rec_doubles(NB, batch)};
    const long rstride = (long)(NB / 64) * BQ_DINV_HALF;
    const bool la = c->cfg.lookahead && c->aux && c->cur == c->stream;
    // df_early: the streams fork BEFORE the panel solve.  The next diagonal block's chain -- the
    // panel solve of ITS rows (the top nw of the panel), its update, its factor -- starts on the
    // second stream at once, beside the solve of the other rows; round 4 forked after the whole
    // panel solve, and in the late blocks the update was shorter than the chain it should hide
    // (C5 shard: 0.11-0.14 ms exposed after three of four blocks, tools/plan_timeline.py).
    const bool early = la && c->cfg.df_early;
    // A factor that has a long update to hide behind (df_wg_rows rows or more below its block) goes
    // to the workgroup-per-matrix kernel whatever the batch: slower alone (366 against 236 us for
    // 64 blocks of 448), but its `batch` workgroups take far fewer slots from the update beside it
    // than the one-launch steps' redundant tiles (C5 shard 5.65 -> 5.57 ms; the first block's
    // factor and the late ones, which nothing hides, stay on the steps)
    auto diag = [&](int K0, int KB, double *rec) {
        if (dfirst_wg(c, batch) ||
            (c->cfg.df_wg < 0 && c->cfg.df_wg_rows > 0 && K0 > 0 && ntot - K0 - KB >= c->cfg.df_wg_rows))
            return launch_potrf_wg(c, A + K0 + (long)K0 * lda, lda, astride, KB, rec, rstride, info,
                                   K0, batch);
        return enqueue_slab_sweep(c, A + K0 + (long)K0 * lda, lda, astride, batch, KB, KB, rec, info,
                                  ws, SweepArgs(), K0, rstride);
    };
    BQCHK(diag(0, NB, recs[0]));
    // while a diagonal factor runs beside an update, gemm_route keeps the rule of a product
    // alone (C5 shard 5.73 ms against 6.05 with the look-ahead's sharing mode 1)
    Sharing scope(c, la ? 0 : c->sharing);
    // The caller assembled only the first NB columns (SweepRoute::seed_cols) and left the rest as a
    // GramSeed: block 0's three products are the first to touch everything right of them, and they
    // compute their tiles of the system instead of loading them -- the assembly of two thirds of a
    // C5 system (an HBM-write-bound launch) and its read-back disappear.
    const bool seeded = a.seed.pts != nullptr;
    auto seed_at = [&](int rr, int cc) {
        GramSeed sd = a.seed;
        sd.r = rr;
        sd.c = cc;
        return sd;
    };
    int par = 0;
    for (int K0 = 0; K0 < ncols; K0 += NB, par ^= 1) {
        const int KB = std::min(NB, ncols - K0), r0 = K0 + KB, m2 = ntot - r0;
        if (m2 <= 0)
            break;
        const double *rec = recs[par];
        const int nw = r0 < ncols ? std::min(NB, ncols - r0) : 0;
        if (nw == 0) {
            BQCHK(enqueue_panel_solve(c, A, lda, astride, batch, r0, m2, K0, KB, rec, rstride,
                                      one_launch));
            // what is left is the Schur complement of the border: nobody reads it when the
            // results come off the border rows
            if (!skip_border)
                BQCHK(launch_gemm(c, BQ_K_SYRK,
                                  trailing_job(A, lda, astride, r0, r0, K0, m2, m2, KB, 1, batch)));
            break;
        }
        const int r1 = r0 + nw;
        if (!early)
            BQCHK(enqueue_panel_solve(c, A, lda, astride, batch, r0, m2, K0, KB, rec, rstride,
                                      one_launch));
        // the next diagonal block: (its rows of the panel solved,) updated and factored -- on the
        // second stream, beside the rest
        if (la) {
            HIPCHK(c, hipEventRecord(c->ev_next, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_next, 0));
        }
        const bool sd0 = seeded && K0 == 0;
        {
            OnStream next(c, la ? c->aux : c->cur);
            if (early) {
                BQCHK(enqueue_panel_solve(c, A, lda, astride, batch, r0, nw, K0, KB, rec, rstride,
                                          one_launch));
                HIPCHK(c, hipEventRecord(c->ev_top, c->aux));
            }
            const GramSeed sd = seed_at(r0, r0);
            GemmJob g = trailing_job(A, lda, astride, r0, r0, K0, nw, nw, KB, 1, batch);
            g.seed = sd0 ? &sd : nullptr;
            BQCHK(launch_gemm(c, BQ_K_SYRK, g));
            BQCHK(diag(r0, nw, recs[par ^ 1]));
        }
        if (la)
            HIPCHK(c, hipEventRecord(c->ev_panel, c->aux));
        if (r1 < ntot) {
            if (early) {
                BQCHK(enqueue_panel_solve(c, A, lda, astride, batch, r1, ntot - r1, K0, KB, rec,
                                          rstride, one_launch));
                // the column update reads the top rows as its Q operand
                HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_top, 0));
            }
            // the rows below it: the next panel's columns, then the square behind them.  (ONE
            // launch over everything right of the panel with the next diagonal block's tiles
            // skipped -- one launch tail instead of two -- was measured in round 5 and gained
            // nothing: C5 5.67 / 256 x C2 4.21 / C3 177-183 either way; removed.  So was the square
            // deferred to every second panel and run once with both panels as its operand, k = 2 NB
            // -- bit-identical results, C5 5.59 / 256 x C2 4.25 / C3 174-176 against 5.60 / 4.21 /
            // 176: what the deeper product gains, the factor that now hides behind the column
            // update alone gives back.)
            const bool sq = !(skip_border && r1 >= ncols);
            const GramSeed sdc = seed_at(r1, r0), sds = seed_at(r1, r1);
            GemmJob col = trailing_job(A, lda, astride, r1, r0, K0, ntot - r1, nw, KB, 0, batch);
            col.seed = sd0 ? &sdc : nullptr;
            BQCHK(launch_gemm(c, BQ_K_SYRK, col));
            if (sq) {
                GemmJob g = trailing_job(A, lda, astride, r1, r1, K0, ntot - r1, ntot - r1, KB, 1, batch);
                g.ccut = skip_border ? ncols - r1 : 0;
                g.seed = sd0 ? &sds : nullptr;
                BQCHK(launch_gemm(c, BQ_K_SYRK, g));
            }
        }
        if (la)
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_panel, 0));
    }
    return BQ_OK;
}

// Eliminate the first r.ncols columns of r.batch matrices along the route sweep_route chose.  ws:
// at least r.ws_doubles of scratch.
int enqueue_potrf_partial(bq_ctx *c, const SweepRoute &r, double *A, long lda, long astride,
                          double *dinv, int *info, double *ws, const SweepArgs &a)
{
    const int batch = r.batch, ntot = r.ntot, ncols = r.ncols;
    if ((ntot & 63) || (ncols & 63) || ncols > ntot)
        return fail(c, BQ_ERR_BAD_ARG, "potrf: sizes must be multiples of 64");
    if (a.seed.pts && r.kind != SweepRoute::DiagFirst)
        return fail(c, BQ_ERR_BAD_ARG, "potrf: a partly assembled system on a sweep that cannot seed it");
    if (r.kind == SweepRoute::Slab)
        return enqueue_slab_sweep(c, A, lda, astride, batch, ntot, ncols, dinv, info, ws, a);
    if (r.kind == SweepRoute::Blocked)
        return enqueue_potrf_group(c, A, lda, astride, batch, ntot, ncols, dinv, info,
                                   r.ws_doubles ? ws : nullptr, r.nb, a.skip_border);
    // (Two half-batches on the two streams, each in lock-step with its diagonal factors on its
    // own stream, were measured in rounds 4 and 5 -- in phase: C5 shard 5.77 ms / 256 x C2 4.33
    // against 5.67 / 4.21 for the whole batch in lock-step; out of phase, the second half
    // starting when the first half's first panel solve is through, so that one half's
    // panel-solve workgroups and diagonal chains run beside the other half's update tiles:
    // 5.87 / 4.52-4.81, C3 186-188 against 177 -- and removed: every launch of a half fills
    // the chip half as well, and two MFMA-bound kernels gain nothing from sharing CUs.)
    if (r.kind == SweepRoute::DiagFirst)
        return enqueue_potrf_dfirst(c, r, A, lda, astride, info, ws, a);
    // Halves: a batch of mid-sized matrices (config C5: 64 x N = 2048) sweeps in lock-step: every
    // 64-column panel step is two short dependent launches that leave most of the chip idle, and a
    // third of the sweep's time is such panel work.  The batch is therefore cut in two halves on
    // the two streams: one half's panel chain runs beside the other half's MFMA trailing update
    // (C5 shard: 7.21 -> 6.78 ms; three or four groups on more streams were slower, 7.8 / 7.5 ms).
    // Both halves keep the whole batch's outer block.
    const int b0 = batch / 2, b1 = batch - b0;
    Sharing halves(c, 2);
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_fork, 0));
    {
        OnStream aux(c, c->aux);
        BQCHK(enqueue_potrf_group(c, A + (long)b0 * astride, lda, astride, b1, ntot, ncols,
                                  dinv + (long)b0 * BQ_DINV_STRIDE, info + b0, nullptr, r.nb,
                                  a.skip_border));
    }
    HIPCHK(c, hipEventRecord(c->ev_panel, c->aux));
    BQCHK(enqueue_potrf_group(c, A, lda, astride, b0, ntot, ncols, dinv, info, nullptr, r.nb,
                              a.skip_border));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_panel, 0));
    return BQ_OK;
}

// One pass over `batch` bordered systems (plan_enqueue, fit_factor): the assembly, the sweep over
// the first L.npad columns and the read-out of log-ML and of the posterior at the M border points.
// sys: the systems' points, targets, kernel parameters and layout; rows: the read-out may come off
// the border rows (plan_readout_kernel); work: the finalize launch's figure for the profiler.
int enqueue_bordered(bq_ctx *c, const GramSeed &sys, int batch, double *A, long lda, long astride,
                     double *dinv, int *info, double *ws, size_t ws_len, double *scal, double *mean,
                     double *var, long mstride, bool rows, double work, long long *stamps,
                     int stamped_steps)
{
    const Layout &L = sys.L;
    const SweepRoute r = sweep_route(c, L.ntot, L.npad, batch, ws_len);
    SweepArgs a;
    a.stamps = stamps;
    a.stamped_steps = stamped_steps;
    // a small system's first sweep launch (and the clearing of the failure flags) rides in
    // the assembly
    FirstStep fs;
    if (r.first_in_assembly) {
        fs.S0 = ws;
        fs.lds = L.ntot;
        fs.sstride = 64L * L.ntot;
        fs.dinv = dinv;
        fs.info = info;
        fs.scal = c->cfg.fold_readout ? scal : nullptr;
        a.first_done = true;
    } else {
        HIPCHK(c, hipMemsetAsync(info, 0, sizeof(int) * batch, c->stream));
    }
    // a batch that sweeps diagonal block first assembles only its first outer block's columns: the
    // first products that touch the rest compute it themselves (GramSeed)
    BQCHK(launch_assemble(c, sys.d, sys.pts, sys.pstride, sys.y, sys.ystride, sys.gp, sys.gpstride,
                          A, lda, astride, L, batch, fs, r.seed_cols));
    if (r.seed_cols > 0)
        a.seed = sys;
    a.skip_border = rows && L.yrow >= 0 && r.border_rows;
    // a sweep of one-launch steps carries the read-out itself (SlabOut: no finalize launch)
    const bool folded = r.first_in_assembly && L.yrow >= 0 && c->cfg.fold_readout;
    if (folded)
        a.out = SlabOut{scal, mean, var, mstride, L.n, L.npad, L.M, L.yrow};
    BQCHK(enqueue_potrf_partial(c, r, A, lda, astride, dinv, info, ws, a));
    if (folded)
        return BQ_OK;
    if (a.skip_border)
        return launch_plan_readout(c, A, lda, astride, L, sys.gp, scal, mean, var, mstride, batch);
    return launch_finalize(c, A, lda, astride, L, scal, mean, var, mstride, batch, work);
}

} // namespace bqh
