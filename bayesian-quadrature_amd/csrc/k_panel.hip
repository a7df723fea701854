// k_panel.hip -- the panel side of the factorisation: assembly of the bordered system (with
// the sweep's first launch folded in), the 64 x 64 diagonal factor, the MFMA panel solve and
// the one-launch steps (gram.h, potf2.h, trsm.h, slab.h), and their launchers.
#include "host.h"
#include "gram.h"
#include "trsm.h"
#include "slab.h"

namespace bqh {

template <int D>
void launch_assemble_d(bq_ctx *c, const double *pts, long pstride, const double *y, long ystride,
                       const GaussParams *gp, int gpstride, double *A, long lda, long astride,
                       Layout L, int batch, const FirstStep &fs, int jcols)
{
    dim3 grid((L.ntot + 127) / 128, ((jcols > 0 ? jcols : L.ntot) + 63) / 64, batch);
    if (!fs.S0) {
        hipLaunchKernelGGL(assemble_kernel<D>, grid, dim3(256), 0, c->cur, pts, pstride, y, ystride,
                           gp, gpstride, A, lda, astride, L);
        return;
    }
    const bool regs = c->cfg.first_regs != 0;
    // (the leading block in registers: workgroup (0, 2) takes rows 64-127 of column block 0 off
    // workgroup (0, 0) -- an idle tile from ntot = 192 on, one more workgroup per problem at
    // ntot = 128: assemble_first_kernel)
    if (regs && grid.y < 3)
        grid.y = 3;
    const long wgs = (long)grid.x * grid.y * grid.z;
    const bool w8 = c->cfg.potf2_8w && wgs <= 2L * c->cus;
#define BQ_ASM_FIRST(NW_, REGS_, STAMP_)                                                           \
    hipLaunchKernelGGL((assemble_first_kernel<D, NW_, REGS_, STAMP_>), grid, dim3(64 * NW_), 0,    \
                       c->cur, pts, pstride, y, ystride, gp, gpstride, A, lda, astride, L, fs.S0,  \
                       fs.lds, fs.sstride, fs.dinv, (long)BQ_DINV_STRIDE, fs.info, fs.scal,        \
                       fs.stamps)
    if constexpr (D == 1) {
        // (the stamped instantiation: the probe's, one dimension)
        if (fs.stamps) {
            if (w8 && regs)
                BQ_ASM_FIRST(8, true, true);
            else if (w8)
                BQ_ASM_FIRST(8, false, true);
            else if (regs)
                BQ_ASM_FIRST(4, true, true);
            else
                BQ_ASM_FIRST(4, false, true);
            return;
        }
    }
    if (w8 && regs)
        BQ_ASM_FIRST(8, true, false);
    else if (w8)
        BQ_ASM_FIRST(8, false, false);
    else if (regs)
        BQ_ASM_FIRST(4, true, false);
    else
        BQ_ASM_FIRST(4, false, false);
#undef BQ_ASM_FIRST
}

int launch_assemble(bq_ctx *c, int d, const double *pts, long pstride, const double *y,
                    long ystride, const GaussParams *gp, int gpstride, double *A, long lda,
                    long astride, Layout L, int batch, const FirstStep &fs, int jcols)
{
    if (jcols < 0 || (jcols & 63) || jcols > L.ntot || (jcols > 0 && fs.S0))
        return fail(c, BQ_ERR_BAD_ARG, "assemble: column limit");
    if (fs.stamps && (!fs.S0 || d != 1))
        return fail(c, BQ_ERR_BAD_ARG, "assemble: the stamped first launch is one-dimensional");
    if (d < 1 || d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    const double cols = jcols > 0 ? jcols : L.ntot;
    Bracket br(c, BQ_K_GRAM, 8.0 * cols * (L.ntot - 0.5 * cols + 0.5) * batch);
    BQ_DISPATCH_D(d, launch_assemble_d<D>(c, pts, pstride, y, ystride, gp, gpstride, A, lda, astride,
                                          L, batch, fs, jcols));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_assemble_region(bq_ctx *c, const GramSeed &sd, double *A, long lda, long astride, int m,
                           int n, int batch)
{
    if (m <= 0 || n <= 0)
        return BQ_OK;
    if ((m & 63) || (n & 63) || (sd.r & 63) || (sd.c & 63))
        return fail(c, BQ_ERR_BAD_ARG, "assemble_region: multiples of 64");
    if (sd.d < 1 || sd.d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    Bracket br(c, BQ_K_GRAM, 8.0 * m * n * batch);
    const dim3 grid((m + 127) / 128, n / 64, batch);
    BQ_DISPATCH_D(sd.d, hipLaunchKernelGGL(assemble_region_kernel<D>, grid, dim3(256), 0, c->cur,
                                           sd.pts, sd.pstride, sd.y, sd.ystride, sd.gp, sd.gpstride,
                                           A, lda, astride, sd.L, sd.r, sd.c, m, n));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_potf2(bq_ctx *c, double *A, long lda, long astride, int j0, double *dinv, long dstride,
                 int *info, int batch)
{
    Bracket br(c, BQ_K_POTF2, 64.0 * 64 * 64 / 3.0 * batch);
    // (eight waves where every matrix of the batch has a CU: potf2f_body<8>)
    if (c->cfg.potf2_8w && batch <= c->cus)
        hipLaunchKernelGGL(potf2_kernel<8>, dim3(1, 1, batch), dim3(512), 0, c->cur, A, lda, astride,
                           j0, dinv, dstride, info);
    else
        hipLaunchKernelGGL(potf2_kernel<4>, dim3(1, 1, batch), dim3(256), 0, c->cur, A, lda, astride,
                           j0, dinv, dstride, info);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// the kb x kb diagonal block of every matrix of a batch, one workgroup per matrix
// (potrf_wg_kernel); rec: kb / 64 records per matrix, rstride doubles apart
int launch_potrf_wg(bq_ctx *c, double *A, long lda, long astride, int kb, double *rec, long rstride,
                    int *info, int col0, int batch)
{
    Bracket br(c, BQ_K_POTF2, (double)kb * kb * kb / 3.0 * batch);
    hipLaunchKernelGGL(potrf_wg_kernel, dim3(batch), dim3(512), 0, c->cur, A, lda, astride, kb, rec,
                       rstride, info, col0);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// the MFMA panel solve (trsm_blk_kernel): needs the block inverses potf2f_body leaves
// behind the 64 reciprocal pivots
int launch_trsm_blk(bq_ctx *c, double *X, long ldx, long xstride, int m, const double *L11,
                    long ldl, long lstride, const double *dinv, long dstride, int batch)
{
    if (m <= 0)
        return BQ_OK;
    Bracket br(c, BQ_K_TRSM, 64.0 * 64 * (double)m * batch);
    hipLaunchKernelGGL(trsm_blk_kernel, dim3((m + 63) / 64, 1, batch), dim3(256), 0, c->cur, X, ldx,
                       xstride, m, L11, ldl, lstride, dinv, dstride);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int launch_diag_winv(bq_ctx *c, const double *L, long ldl, int npad, double *dw)
{
    hipLaunchKernelGGL(diag_winv_kernel, dim3(npad / 64), dim3(256), 0, c->stream, L, ldl, dw);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// one step of a wide panel in one launch (panel_step_kernel, slab.h)
int launch_panel_step(bq_ctx *c, double *A, long lda, long astride, int batch, int nrb,
                      double *Sin, double *Sout, long lds, long sstride, int K0, int j0,
                      double *dinv_in, double *dinv_out, int has_next, int first, double *SL,
                      int *info, double work)
{
    Bracket br(c, BQ_K_GEMM, work);
    // Eight waves where every workgroup of the step has a CU to itself: the second row-block
    // solve and the next diagonal factor on waves 4-7.  Not beside a look-ahead's bulk update
    // (sharing): eight waves of 244 VGPRs need a CU's whole register file, which no retiring
    // workgroup of the update frees -- N = 16384 lost 2.5 us per step, 0.65 ms, to the wait.
    // The update occupies the chip for about m^2 NB / 50 TFLOP/s and the panel's chain lasts
    // NB / 64 x 21 us: from m = 4,000 rows down (64 row blocks) the chain out-lasts the update
    // it sits beside, finds free CUs for most of its steps, and takes the eight waves again.
    const bool beside_bulk = c->sharing != 0 && (long)nrb * batch > 64;
    if (c->cfg.potf2_8w && !beside_bulk && (long)nrb * batch <= c->cus)
        hipLaunchKernelGGL(panel_step_kernel<8>, dim3(nrb, 1, batch), dim3(512), 0, c->cur, A, lda,
                           astride, Sin, Sout, lds, sstride, K0, j0, dinv_in, dinv_out,
                           (long)BQ_DINV_STRIDE, has_next, first, SL, info);
    else
        hipLaunchKernelGGL(panel_step_kernel<4>, dim3(nrb, 1, batch), dim3(256), 0, c->cur, A, lda,
                           astride, Sin, Sout, lds, sstride, K0, j0, dinv_in, dinv_out,
                           (long)BQ_DINV_STRIDE, has_next, first, SL, info);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// the first diagonal factor of a slab sweep and the staging of panel 0 in one launch
int launch_slab_first(bq_ctx *c, double *A, long lda, long astride, int batch, double *S, long lds,
                      long sstride, int ntot, double *dinv, int *info, int col0, long dstride)
{
    Bracket br(c, BQ_K_POTF2, 64.0 * 64 * 64 / 3.0 * batch);
    hipLaunchKernelGGL(slab_first_kernel, dim3(ntot / 64, 1, batch), dim3(256), 0, c->cur, A, lda,
                       astride, S, lds, sstride, ntot, dinv, dstride, info, col0);
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// The most workgroups a step may have and still run in its 512-thread form: slab8_rounds rounds of
// one workgroup per CU.  (Its waves 4-7 work in every tile: in an off-diagonal tile they solve the
// Q rows, in a diagonal tile they update it behind the solve's column blocks -- slab.h, PIPE.)
// Shipped: no limit -- us per step, 512 / 256 threads (tools/slab_step_time.py, medians of 7;
// profiles/diagpipe_slab_step_time.txt; LABBOOK, "A diagonal tile's update under its solve"):
//     workgroups      one matrix         5 x N = 1024      16 x N = 768
//        ~50        15.0 / 17.0        15.6 / 19.8        16.5 / 18.7
//        ~250       17.0 / 18.4        18.3 / 21.6        19.0 / 21.8
//        ~280       20.5 / 22.2        21.2 / 22.7        24.8 / 27.4 (336)
//        ~500       21.5 / 23.2        25.4 / 28.3        23.7 / 26.3
//        ~600       25.7 / 26.8        26.6 / 29.1        27.5 / 29.8
//        ~950       32.6 / 33.8             --            38.4 / 42.9
//        ~2150      55.1 / 54.3             --                 --
//        ~2550      53.1 / 53.3             --                 --
// The 512-thread form is 0.8 - 2.0 us ahead up to 1,000 workgroups (more in a stacked batch) and
// level from 1,700 (within +-0.8 us, either way); the 3 - 4 us a step gains with every 256
// workgroups are the same in both.  (Measured again, parent against branch, when the kernel became
// a dispatcher over named tile paths: 512-thread medians of one matrix -0.4 ... +0.5 us, mean +0.05 us;
// of 5 x N = 1024 -0.2 ... +1.0 us with minima within +-0.3 us (a median of 7 carries outliers there,
// in either build).  One matrix lies inside the +-0.8 us above and the 256-thread column moved as
// much: the table stands -- profiles/solve16_slab_step_time.txt; LABBOOK, "One 16-row block-inverse
// solve".)
static long slab8_limit(const bq_ctx *c)
{
    return (long)(c->cfg.slab8_rounds > 1 ? c->cfg.slab8_rounds : 1) * c->cus;
}

// one 64-column step of a small system in one launch (slab_step_kernel); out: the read-out the
// last step stores (SlabOut); stamps: the profiling instantiation (bq_probe_c2_timeline)
int launch_slab_step(bq_ctx *c, double *A, long lda, long astride, int batch, double *Sin,
                     double *Sout, long lds, long sstride, int ntot, int j0, double *dinv_in,
                     double *dinv_out, int fnext, int last, int *info, int col0,
                     const SlabOut &out, long long *stamps, double work, long dstride)
{
    const int T = (ntot - j0 - 64) / 64;
    Bracket br(c, BQ_K_SYRK_SMALL, work);
    const long wgs = (long)T * (T + 1) / 2 * batch;
    // (the last step -- no next factor, the Schur complement of the border -- too: its
    // off-diagonal workgroups solve their two row blocks side by side; waves 4-7 leave after the
    // Q rows' barrier and waves 0-3 store and emit as in the four-wave form)
    const bool w8 = c->cfg.potf2_8w && wgs <= slab8_limit(c);
    // (512 threads: both row-block solves at once, the diagonal factor on eight waves, and --
    // diag_pipe -- a diagonal tile's update on waves 4-7 behind the solve's column blocks)
    const bool pipe = w8 && c->cfg.diag_pipe != 0;
    // (write-through tile stores, tile_wt: where all workgroups of the step run in ONE round, every
    // tile but workgroup 0's is done long before workgroup 0 leaves its pivot chain, and what its
    // stores leave dirty in the L2s is written back at the kernel's end, in front of the next step.
    // In a step of several rounds or a stacked batch the stores are throughput and stay plain; so
    // does the last step, which has no chain to hide them under.)
    const bool wt = w8 && c->cfg.tile_wt != 0 && fnext && wgs <= c->cus;
    // (the last step of a sweep that carries its read-out emits it and stores no tile)
    const bool emit = last && out.scal != nullptr;
#define BQ_SLAB_STEP(STAMP_, NW_, PIPE_, TILES_)                                                   \
    hipLaunchKernelGGL((slab_step_kernel<STAMP_, NW_, PIPE_, TILES_>),                             \
                       dim3(T * (T + 1) / 2, 1, batch), dim3(64 * NW_), 0, c->cur, A, lda,         \
                       astride, Sin, Sout, lds, sstride, ntot, j0, dinv_in, dinv_out, dstride,     \
                       fnext, last, info, col0, STAMP_ ? stamps : (long long *)nullptr, out)
#define BQ_SLAB_STEP_NW(STAMP_, NW_, PIPE_)                                                        \
    do {                                                                                           \
        if (emit)                                                                                  \
            BQ_SLAB_STEP(STAMP_, NW_, PIPE_, SLAB_TILES_EMIT);                                     \
        else if (NW_ == 8 && wt)                                                                   \
            BQ_SLAB_STEP(STAMP_, 8, PIPE_, SLAB_TILES_WT);                                         \
        else                                                                                       \
            BQ_SLAB_STEP(STAMP_, NW_, PIPE_, SLAB_TILES_PLAIN);                                    \
    } while (0)
#define BQ_SLAB_STEP_ANY(STAMP_)                                                                   \
    do {                                                                                           \
        if (pipe)                                                                                  \
            BQ_SLAB_STEP_NW(STAMP_, 8, true);                                                      \
        else if (w8)                                                                               \
            BQ_SLAB_STEP_NW(STAMP_, 8, false);                                                     \
        else                                                                                       \
            BQ_SLAB_STEP_NW(STAMP_, 4, false);                                                     \
    } while (0)
    if (stamps)
        BQ_SLAB_STEP_ANY(true);
    else
        BQ_SLAB_STEP_ANY(false);
#undef BQ_SLAB_STEP_ANY
#undef BQ_SLAB_STEP_NW
#undef BQ_SLAB_STEP
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

} // namespace bqh
