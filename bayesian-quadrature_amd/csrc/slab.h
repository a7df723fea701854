// slab.h -- one launch per 64-column step of a small factorisation (outer block 64)
// Part of the libbqhip.so kernel set; compiled into k_panel.hip (host.h lists the units).
#pragma once
#include "common.h"
#include "potf2.h"
#include "solve16.h"

// ---------------------------------------------------------------------------
// Small systems (one 64-column slab per outer step: C2, the reference's own problem
// sizes, the batched active-sampling systems) are a chain of dependent launches; every
// step used to be three of them -- trailing update (+ fused diagonal factor), panel
// solve -- and the chain, not the arithmetic, is the time.  Here a step is ONE launch and
// nothing in it waits on another workgroup:
//
//   the workgroup of trailing tile (bx, by) solves the panel rows it needs ITSELF --
//   row block bx and row block by, 64 x 64 each, on the matrix cores from the 16 x 16
//   block inverses potf2 left behind (the trsm_blk_kernel scheme, 40 MFMAs per wave) --,
//   updates its tile with them, and workgroup (0, 0) then factors the next diagonal block.
//
// The solve is recomputed by every workgroup that needs the rows (at most 2 x 80 MFMAs
// per wave, nothing next to a launch).  The unsolved panel cannot be overwritten in place
// while other workgroups still read it, so it lives in a scratch column: the step reads
// its panel from Sin and the workgroups of tile column 0 -- the next panel -- write their
// updated tiles to Sout (ping-pong) instead of A; workgroup (bx, 0) also writes the
// solved rows, the final L, to A.  The reciprocal pivots / block inverses ping-pong the
// same way (workgroup 0 writes the next block's while others may still read this one's).
//
//   A      ntot x ntot, column-major; L_jj at (j0, j0) factored by the previous launch
//   Sin    unsolved panel column j0 for rows >= j0 + 64, absolute row index, ld lds
//   Sout   receives the next panel column (rows >= j0 + 128) unless `last`
//   din    64 reciprocal pivots + 4 block inverses of L_jj; dout: the same for the next block
//   factor_next: workgroup (0, 0) factors the diagonal block at j0 + 64 after updating it
// grid: (T (T + 1) / 2, 1, batch), T = (ntot - j0 - 64) / 64; block 256.
// ---------------------------------------------------------------------------

// The ten lower 16 x 16 blocks (rb, cb) of a diagonal tile dealt to the four waves:
//   wave 0: (0,0) (1,0) (1,1)   wave 1: (2,0) (2,1) (2,2)   wave 2: (3,0) (3,1)   wave 3: (3,2) (3,3)
// Every wave issues THREE MFMAs per k-step: waves 2 and 3 repeat their second block into an
// accumulator that is never stored.  (A third MFMA under `if (wave < 2)` was miscompiled into
// a wrong block (3, 1): an MFMA ignores EXEC, so it must never sit under anything but a scalar
// branch, and the redundant one costs nothing -- the other two waves issue three anyway.)
__device__ __forceinline__ constexpr int slab_diag_nb(int w) { return w < 2 ? 3 : 2; }
__device__ __forceinline__ constexpr int slab_diag_rb(int w, int s)
{
    return w == 0 ? (s > 0 ? 1 : 0) : (w == 1 ? 2 : 3);
}
__device__ __forceinline__ constexpr int slab_diag_cb(int w, int s)
{
    return w == 0 ? (s == 2 ? 1 : 0) : ((w == 3 ? 2 : 0) + (w >= 2 && s == 2 ? 1 : s));
}

// What a workgroup of slab_step_kernel knows about itself, handed by value to the tile paths
// below: the batch-offset pointers, the tile, the wave number, the kernel's flags.  (Lane numbers:
// mfma_l15 / mfma_l4, solve16.h.)
struct SlabWg {
    double *A;
    const double *Sin;
    double *Sout;
    const double *din;
    double *dout;
    long lda, lds;
    int j0, r0, Rb, Cb, bx, by, wave, b, factor_next, last, col0;
    int swg; // (STAMP: the off-diagonal workgroup that stamps its stores, BQ_SSTAMP_STORES)
    int *info;
    long long *stamps;
    // The kernel's own argument, by reference: by value its fields sit in SGPRs across the whole
    // kernel.  WHOEVER READS out's fields in a loop copies it first (`const SlabOut o = g.out`, as
    // slab_store_diag does): through the reference every entry re-reads them behind its stores.
    const SlabOut &out;
};

// A wave's solved 16 rows (rows 16 w .. + 15 of the tile's 64) into the Q rows, [k][row]: column
// block c as it comes, or all four
__device__ __forceinline__ void slab_publish_block(double *Qs, int c, int w, int l15, int l4,
                                                   const double4_t &xc)
{
#pragma unroll
    for (int r = 0; r < 4; ++r)
        Qs[(16 * c + l4 + 4 * r) * 64 + 16 * w + l15] = xc[r];
}

__device__ __forceinline__ void slab_publish(double *Qs, int w, int l15, int l4,
                                             const double4_t (&x)[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c)
        slab_publish_block(Qs, c, w, l15, l4, x[c]);
}

// The last step's tiles are the Schur complement S of the border: with the read-out folded
// in (SlabOut) the lane that holds S[c, c], S[yrow, c] or S[yrow, yrow] stores var_i, mean_i
// and -- log|K| is complete since the previous launch -- the log-ML (reduce.h,
// finalize_kernel, is the stand-alone form).  row / col: this sweep's numbering = the
// system's (col0 = 0 for every caller that sets `out`).
__device__ __forceinline__ void slab_emit(const SlabOut &out, int b, int row, int col, double s)
{
    if (row == col && row >= out.npad && row < out.npad + out.M && out.var)
        out.var[(long)b * out.mstride + (row - out.npad)] = s;
    if (row == out.yrow) {
        if (col >= out.npad && col < out.npad + out.M && out.mean)
            out.mean[(long)b * out.mstride + (col - out.npad)] = -s;
        if (col == out.yrow) {
            const double qf = -s, ld = out.scal[4 * b + 1];
            out.scal[4 * b + 2] = qf;
            out.scal[4 * b + 0] = -0.5 * qf - 0.5 * ld - 0.5 * (double)out.n * 1.8378770664093453;
        }
    }
}

// What a step does with its updated tiles (slab_step_kernel's TILES; launch_slab_step has the rule):
//   SLAB_TILES_PLAIN  plain stores.  The code of the steps before there were modes, instruction for
//                     instruction, its own read-out branch included, which is never taken any more
//                     (launch_slab_step sends every folded last step to SLAB_TILES_EMIT): without it
//                     hipcc schedules the update of workgroup 0 differently and a step is 0.1 us
//                     longer (LABBOOK, "The tiles' way to memory").
//   SLAB_TILES_WT     write-through stores (launch_config.h, tile_wt): the line leaves the XCD's L2
//                     when it is stored, under workgroup 0's pivot chain, instead of standing dirty
//                     until the kernel's end, where its write-back is the next launch's wait.  Same
//                     value, same address; no workgroup of a launch reads what another one stores,
//                     so nothing is ordered by it.  The tiles of workgroups 1 and 2 -- (1, 0), the
//                     next panel's first rows, and (1, 1), the next diagonal block: what the next
//                     launch's workgroup 0 loads first -- stay plain: 52 KB.
//   SLAB_TILES_EMIT   the last step with the read-out folded in: slab_emit takes what anybody reads
//                     of its tiles (the Schur complement of the border), so the tiles are not
//                     stored, and an off-diagonal tile without the y row that is not in tile column
//                     0 (whose workgroups store the solved border rows) is not computed: its
//                     workgroup returns at entry (slab_tile_dead).
enum { SLAB_TILES_PLAIN = 0, SLAB_TILES_WT = 1, SLAB_TILES_EMIT = 2 };

template <int TILES>
__device__ __forceinline__ void slab_tile_store(double *p, double v, bool wt)
{
    static_assert(TILES != SLAB_TILES_EMIT, "the folded last step stores no tile");
    if (TILES == SLAB_TILES_WT && wt)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}

// (write-through in this workgroup: wave-uniform)
__device__ __forceinline__ bool slab_wg_wt() { return blockIdx.x > 2; }

__device__ __forceinline__ bool slab_tile_dead(const SlabOut &out, int bx, int by, int Rb)
{
    return bx != by && by > 0 && (out.yrow < Rb || out.yrow >= Rb + 64);
}

// (does this step emit the read-out: a constant but in SLAB_TILES_PLAIN)
template <int TILES>
__device__ __forceinline__ bool slab_emits(const SlabWg &g)
{
    if constexpr (TILES == SLAB_TILES_PLAIN)
        return g.last && g.out.scal != nullptr;
    return TILES == SLAB_TILES_EMIT;
}

// Wave w's blocks of an updated diagonal tile (-acc: the accumulators hold the negated tile)
// back to A, or (SLAB_TILES_EMIT) the read-out of the last step
template <int TILES, int NA>
__device__ __forceinline__ void slab_store_diag(const SlabWg &g, int w, const double4_t (&acc)[NA])
{
    const int l15 = mfma_l15(), l4 = mfma_l4();
    const bool wt = slab_wg_wt();
    const bool emit = slab_emits<TILES>(g);
#pragma unroll
    for (int sb = 0; sb < 3; ++sb)
        if (sb < slab_diag_nb(w)) {
            double *Cd = g.A + g.Rb + 16 * slab_diag_rb(w, sb) + l15 +
                         (long)(g.Cb + 16 * slab_diag_cb(w, sb) + l4) * g.lda;
            if constexpr (TILES != SLAB_TILES_EMIT) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    slab_tile_store<TILES>(Cd + (long)(4 * r) * g.lda, -acc[sb][r], wt);
            }
            if (emit) {
                const SlabOut o = g.out; // (by value: every field is read once, not per entry)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    slab_emit(o, g.b, g.Rb + 16 * slab_diag_rb(w, sb) + l15,
                              g.Cb + 16 * slab_diag_cb(w, sb) + l4 + 4 * r, -acc[sb][r]);
            }
        }
}

// Workgroup 0 of an eight-wave step hands the updated diagonal block to the factor as its ten
// lower 16 x 16 blocks, packed: block (rb, cb), cb <= rb, at 256 (rb (rb + 1) / 2 + cb), element
// (i, k) at i + 16 k -- BQ_SLAB_FW doubles, exactly the fragment region, which is dead once every
// wave holds its fragments.  Wave w's blocks go in ...
template <int NA>
__device__ __forceinline__ void slab_pack_blocks8(double *Bs, int w,
                                                  const double4_t (&acc)[NA])
{
    const int l15 = mfma_l15(), l4 = mfma_l4();
#pragma unroll
    for (int sb = 0; sb < 3; ++sb)
        if (sb < slab_diag_nb(w)) {
            const int rb = slab_diag_rb(w, sb), cb = slab_diag_cb(w, sb);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Bs[256 * ((rb * (rb + 1)) / 2 + cb) + l15 + 16 * (l4 + 4 * r)] = -acc[sb][r];
        }
}

// ... and every wave of the factor picks its columns out of them, row `lane`; a lane above a
// column's own block row takes 0.0, which the factor never reads.
__device__ __forceinline__ void slab_load_blocks8(Potf2FT<8> &st, const double *Bs, int w, int lane)
{
    const int rb = lane >> 4, i = lane & 15;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int c = 4 * (8 * q + w) + s; // (potf2.h: panel 8 q + w is this wave's group q)
            const int cb = c >> 4, rc = rb > cb ? rb : cb;
            const double v = Bs[256 * ((rc * (rc + 1)) / 2 + cb) + i + 16 * (c & 15)];
            st.a[q][s] = rb >= cb ? v : 0.0;
        }
}

// ... and factors it: behind ONE barrier after the blocks were written.  Nobody reads the Q rows
// any more, so the first panel may be published into their place at once.
__device__ __forceinline__ void slab_corner_factor8(double *Ab, long lda, int j0, double *dinv_b,
                                                    int *info_b, double *plds, long long *stamps,
                                                    double *logdet)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (stamps && threadIdx.x == 0)
        stamps[0] = (long long)__builtin_amdgcn_s_memtime();
    Potf2FT<8> st;
    slab_load_blocks8(st, plds + 4096, w, lane);
    potf2f_run<8>(st, Ab, lda, j0, dinv_b, info_b, plds, stamps, logdet);
}

// (the step's call of it: the diagonal block at r0 of this problem; stamps: the factor's own)
__device__ __forceinline__ void slab_factor_next8(const SlabWg &g, double *plds, long long *stamps)
{
    slab_corner_factor8(g.A + g.r0 + (long)g.r0 * g.lda, g.lda, g.col0 + g.r0, g.dout, g.info + g.b,
                        plds, stamps, g.out.scal ? g.out.scal + 4 * g.b + 1 : nullptr);
}

// STAMP: a profiling instantiation (tools/c2_timeline.py) whose workgroup 0 records s_memtime
// at its phase boundaries; the shipped launches use STAMP = false and carry no stamp code.
// tid: the thread of workgroup 0 that records (wave 4's lane 0 is thread 256).
#define BQ_SSTAMP_AT(stamps_, k, dep, wg, tid, clock)                                              \
    if (STAMP) {                                                                                   \
        asm volatile("" ::"v"(dep));                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        if ((int)blockIdx.x == (wg) && blockIdx.z == 0 && threadIdx.x == (tid))                    \
            (stamps_)[k] = (long long)clock();                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                         \
    }
#define BQ_SSTAMP(stamps_, k, dep, tid)                                                            \
    BQ_SSTAMP_AT(stamps_, k, dep, 0, tid, __builtin_amdgcn_s_memtime)
// Slots 24 .. 31: the stores.  s_memtime counts per XCD, so what is compared ACROSS workgroups is
// s_memrealtime (100 MHz, one counter): [24] / [25] workgroup 0 at entry / at its last instruction,
// which with [0] and the factor's stamps places every phase of it on that clock; [26] / [27] /
// [28] one off-diagonal workgroup (g.swg: the last tile row's second tile, which also the last
// step keeps) at entry / behind its update / with its tile's stores acknowledged; [29] .. [31] the
// same workgroup's s_memtime at the same three places.  `drained`: the wait for the stores.
#define BQ_SSTAMP_STORES(stamps_, k, dep, wg, tid, drained)                                        \
    if (STAMP) {                                                                                   \
        if (drained)                                                                               \
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                       \
        BQ_SSTAMP_AT(stamps_, k, dep, wg, tid, __builtin_amdgcn_s_memrealtime)                     \
        if ((wg) != 0)                                                                             \
            BQ_SSTAMP_AT(stamps_, (k) + 3, dep, wg, tid, __builtin_amdgcn_s_memtime)               \
    }

// --- the tile paths of slab_step_kernel, one per row group of the barrier table in front of it ---

// Table rows "diagonal, NW = 8, PIPE", waves 4-7: A B0 B1 B2 B3 [F + factor].
// diagonal tile: the update is THIS group's.  The ten lower blocks, dealt 3 / 3 / 2 / 2 by
// slab_diag_rb / slab_diag_cb of wave - 4 and requested RAW before the first barrier; the
// two-block waves load and update their second block again as a third, which nothing stores (an
// MFMA ignores EXEC).
template <bool STAMP, int TILES>
__device__ __forceinline__ void slab_pipe_update(const SlabWg g, double *plds)
{
    double *const Qs = plds;
    const int l15 = mfma_l15(), l4 = mfma_l4();
    __builtin_assume(g.wave >= 4); // (the dispatch's condition, lost behind the call)
    const int wu = g.wave - 4;
    const int rb0 = slab_diag_rb(wu, 0), rb1 = slab_diag_rb(wu, 1), rb2 = slab_diag_rb(wu, 2);
    const int cb0 = slab_diag_cb(wu, 0), cb1 = slab_diag_cb(wu, 1), cb2 = slab_diag_cb(wu, 2);
    double4_t acc[3];
#pragma unroll
    for (int sb = 0; sb < 3; ++sb) {
        const double *Cin = g.A + g.Rb + 16 * slab_diag_rb(wu, sb) + l15 +
                            (long)(g.Cb + 16 * slab_diag_cb(wu, sb) + l4) * g.lda;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[sb][r] = Cin[(long)(4 * r) * g.lda];
    }
    __syncthreads(); // A
    // negated behind the first barrier: nothing needs the tile before x_0 is published
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sb = 0; sb < 3; ++sb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = -acc[sb][r];
            asm volatile("" : "+v"(v));
            acc[sb][r] = v;
        }
    __builtin_amdgcn_sched_barrier(0);
    // k-block c behind the barrier that publishes x_c: block (rb, cb) += X_cb X_rb^T in
    // D^T form, the MFMAs of every accumulator in the order c, r of the one-phase update;
    // all 24 LDS operands of the k-block are requested before its first MFMA
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c > 0)
            BQ_SSTAMP(g.stamps, 15 + c, acc[0][0], 256) // wave 4 arrives at B_c
        // (pinned: left alone, the scheduler sinks eleven of a k-block's MFMAs behind
        // the next barrier, and two k-blocks instead of one stand behind the solve)
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads(); // B_c
        __builtin_amdgcn_sched_barrier(0);
        double qa[4][3], qb[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double *qrow = Qs + (16 * c + l4 + 4 * r) * 64 + l15;
            qa[r][0] = qrow[16 * cb0], qb[r][0] = qrow[16 * rb0];
            qa[r][1] = qrow[16 * cb1], qb[r][1] = qrow[16 * rb1];
            qa[r][2] = qrow[16 * cb2], qb[r][2] = qrow[16 * rb2];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[r][0], qb[r][0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[r][1], qb[r][1], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[r][2], qb[r][2], acc[2], 0, 0, 0);
        }
    }
    BQ_SSTAMP(g.stamps, 4, acc[1][3] + acc[0][0], 256)
    if (blockIdx.x == 0 && g.factor_next) {
        // the packed blocks go where the fragments were: waves 0-3 took their last
        // fragments in front of B_3
        slab_pack_blocks8(plds + 4096, wu, acc);
        __syncthreads(); // F
        slab_factor_next8(g, plds, nullptr);
        return;
    }
    slab_store_diag<TILES>(g, wu, acc);
    BQ_SSTAMP_STORES(g.stamps, 25, 0, 0, 256, true) // (workgroup 0 stores a tile in the last step only)
}

// Column block C of the pipelined solve: x_C published in the Q rows the moment it exists, a
// barrier behind it (B_C); the fragments of column block C + 2 are requested in front of B_C,
// so that no LDS round trip stands between a barrier and the chain (the last ones in front of
// B_1: waves 4-7 overwrite the fragment region behind B_3).
template <bool STAMP, int C>
__device__ __forceinline__ void slab_pipe_block(const SlabWg &g, double *plds, const double (&tc)[4],
                                                Solve16Regs<> &f, double4_t (&x)[4])
{
    solve16_block<C>(tc, f, x);
    slab_publish_block(plds, C, g.wave, mfma_l15(), mfma_l4(), x[C]);
    if constexpr (C < 2)
        f.template load_lds_block<C + 2>(plds + 4096);
    if (C > 0)
        BQ_SSTAMP(g.stamps, 18 + C, x[C][3], 0) // wave 0 arrives at B_c
    // (not pinned: hipcc moves the MFMAs of x_{c+1} up in front of B_c and only
    // its ds_write behind it; pinned to 4 / 8 / 12 / 16 MFMAs per interval the
    // update waits less and the headline is the same: LABBOOK)
    __syncthreads(); // B_c
}

// Table rows "diagonal, NW = 8, PIPE", waves 0-3: A B0 B1 B2 B3 [F + factor].
// The fragments of L_jj and W staged once per workgroup and the panel rows, as in the one-phase
// prologue -- but no C tile: that is waves 4-7's.  A path of its own from its first load to its
// return (ONE prologue with a branch behind barrier A cost 254 VGPRs and spills: LABBOOK); it
// shares the staging, the fragments and the solve with the one-phase body through solve16.h.
template <bool STAMP>
__device__ __forceinline__ void slab_pipe_solve(const SlabWg g, double *plds)
{
    const int l15 = mfma_l15(), l4 = mfma_l4();
    double tp[4][4];
    double *Fs = plds + 4096;
    {
        double f6[6], wv[4];
        solve16_stage_request(g.A + g.j0 + (long)g.j0 * g.lda, g.lda, g.din, f6, wv);
        solve16_load(g.Sin + g.Rb + 16 * g.wave + l15 + (long)l4 * g.lds, g.lds, tp);
        // nothing that waits for a load may move up between the loads
        __builtin_amdgcn_sched_barrier(0);
        solve16_stage_store(Fs, f6, wv);
    }
    __syncthreads(); // A
    Solve16Regs<> f;
    double4_t x[4];
    f.load_lds_block<0>(Fs);
    f.load_lds_block<1>(Fs);
    BQ_SSTAMP(g.stamps, 1, f.wf[0][3] + f.wf[1][3], 0)
    slab_pipe_block<STAMP, 0>(g, plds, tp[0], f, x);
    slab_pipe_block<STAMP, 1>(g, plds, tp[1], f, x);
    slab_pipe_block<STAMP, 2>(g, plds, tp[2], f, x);
    slab_pipe_block<STAMP, 3>(g, plds, tp[3], f, x);
    BQ_SSTAMP(g.stamps, 2, x[3][3], 0)
    // the solved rows are the factor: tile column 0 owns the write
    if (g.by == 0)
        solve16_store(g.A + g.Rb + 16 * g.wave + l15 + (long)(g.j0 + l4) * g.lda, g.lda, x);
    if (blockIdx.x == 0 && g.factor_next) {
        __syncthreads(); // F
        slab_factor_next8(g, plds, (STAMP && blockIdx.z == 0) ? g.stamps + 5 : nullptr);
        BQ_SSTAMP_STORES(g.stamps, 25, 0, 0, 0, false)
    }
}

// Table rows "off-diagonal tile", waves 4-7: A Q; and "diagonal, NW = 8, !PIPE", waves 4-7:
// A Q [F + factor] -- the barriers of the one-phase body below, in their order: fragments
// staged; Q rows written; and for workgroup 0 with a next factor: diagonal block in LDS.
__device__ __forceinline__ void slab_upper_waves(const SlabWg g, double *plds)
{
    const int l15 = mfma_l15(), l4 = mfma_l4();
    if (g.bx != g.by) {
        // off-diagonal tile: the Q rows (row block by) are solved HERE, beside waves 0-3's
        // solve of the P rows -- the two are independent, and one after the other they were
        // 2 x 3,300 cycles of every such workgroup.  Same MFMAs on the same operands in the
        // same order as the four-wave form does them on waves 0-3.
        __builtin_assume(g.wave >= 4); // (the dispatch's condition, lost behind the call)
        const int wq = g.wave - 4;
        double tq[4][4];
        solve16_load(g.Sin + g.Cb + 16 * wq + l15 + (long)l4 * g.lds, g.lds, tq);
        __syncthreads();
        Solve16Regs<> f;
        f.load_lds(plds + 4096);
        double4_t xq[4];
        solve16(tq, f, xq);
        slab_publish(plds, wq, l15, l4, xq);
        __syncthreads();
        return; // (workgroup 0 is a diagonal tile)
    }
    __syncthreads();
    __syncthreads();
    if (blockIdx.x == 0 && g.factor_next) {
        __syncthreads();
        slab_factor_next8(g, plds, nullptr);
    }
}

// The update of a one-phase diagonal tile, both operands from LDS (Q = P here): block (rb, cb)
// += X_cb X_rb^T in D^T form.  D[n][i] = sum_k Q[n][k] P[i][k], C -= D^T.
__device__ __forceinline__ void slab_update_diag(const double *Qs, int wave,
                                                 double4_t (&acc)[4])
{
    const int l15 = mfma_l15(), l4 = mfma_l4();
    const int rb0 = slab_diag_rb(wave, 0), rb1 = slab_diag_rb(wave, 1), rb2 = slab_diag_rb(wave, 2);
    const int cb0 = slab_diag_cb(wave, 0), cb1 = slab_diag_cb(wave, 1), cb2 = slab_diag_cb(wave, 2);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double *qrow = Qs + (16 * c + l4 + 4 * r) * 64 + l15;
            acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(qrow[16 * cb0], qrow[16 * rb0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(qrow[16 * cb1], qrow[16 * rb1], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(qrow[16 * cb2], qrow[16 * rb2], acc[2], 0, 0, 0);
        }
}

// ... and of an off-diagonal one: A operand = Q fragment from LDS, B operand = P as it stands
__device__ __forceinline__ void slab_update_offdiag(const double *Qs,
                                                    const double4_t (&xp)[4], double4_t (&acc)[4])
{
    const int l15 = mfma_l15(), l4 = mfma_l4();
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double pf = xp[c][r];
            const double *qrow = Qs + (16 * c + l4 + 4 * r) * 64 + l15;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(qrow[16 * cb], pf, acc[cb], 0, 0, 0);
        }
}

// Table rows "off-diagonal tile", waves 0-3: A Q; "diagonal, NW = 4": A Q [T F + factor];
// "diagonal, NW = 8, !PIPE", waves 0-3: A Q [F + factor] -- the one-phase body (four waves, or
// waves 0-3 of eight).
template <bool STAMP, int NW, bool PIPE, int TILES>
__device__ __forceinline__ void slab_one_phase(const SlabWg g, double *plds)
{
    double *const Qs = plds;
    double *const Ts = plds; // the block sits where the factor's panel slots will be
    double *const Fs = plds + 4096;
    const int bx = g.bx, by = g.by, wave = g.wave, l15 = mfma_l15(), l4 = mfma_l4();
    // Every global load of the step is issued here, before the first MFMA: the fragments of
    // L_jj (blocks below its diagonal) and of the negated block inverses, the unsolved panel
    // rows of both row blocks and the C tile.  (Loaded where they are first used, the tile
    // waited behind the factor's stores, which may alias it, and the launch paid three
    // memory round trips one after the other.)
    Solve16Regs<> f;
    double tp[4][4], tq[4][4];
    double4_t acc[4];
    {
        // The fragments of L_jj and W are the same for all four waves: the workgroup fetches
        // the six 16 x 16 blocks below L_jj's diagonal and the four block inverses ONCE into
        // LDS (10 doubles per thread; the region is the diagonal factor's, free until the
        // tile update is over) instead of 64 doubles per lane from L2 -- a CU takes in about
        // 40 B per cycle and the fragment loads were half of the launch's 190 KB.
        double f6[6], wv[4];
        solve16_stage_request(g.A + g.j0 + (long)g.j0 * g.lda, g.lda, g.din, f6, wv);
        // No branch between the loads either: a load under `if` is a basic block of its own,
        // and hipcc puts the waits of the OTHER arm's pending loads in front of it.  So the
        // four-wave form loads the Q rows in a diagonal tile too (they are its P rows: the
        // same lines), and the C tile's sixteen loads differ between the two kinds of tile
        // only in wave-uniform offsets.
        if (NW == 4)
            solve16_load(g.Sin + g.Cb + 16 * wave + l15 + (long)l4 * g.lds, g.lds, tq);
        solve16_load(g.Sin + g.Rb + 16 * wave + l15 + (long)l4 * g.lds, g.lds, tp);
        // C tile, RAW: the MFMAs add Q P^T to -C, but a negation here draws the load's wait
        // in between the loads (the scheduler places the sign flip as early as it may) and
        // the tile then costs one memory round trip per group of loads; it is negated in
        // front of the update instead.  Off-diagonal tiles: rows 16 wave .. +15,
        // four 16-column blocks.  Diagonal tiles need only their ten lower 16 x 16 blocks
        // and deal them 3 / 3 / 2 / 2 to the waves (slab_diag_rb / slab_diag_cb): 48 MFMAs on
        // the longest wave instead of 64 -- for workgroup (0, 0) this update sits between the
        // launch's start and the diagonal factor.  Waves 2 and 3 load their second block
        // again as a third (s = 2, as for the MFMAs: never stored), and every wave of a
        // diagonal tile loads its third block again as a fourth, which nothing reads.
        {
            const bool dg = bx == by;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const int sb = cb < 2 ? cb : 2;
                const int ro = dg ? 16 * slab_diag_rb(wave, sb) : 16 * wave;
                const int co = dg ? 16 * slab_diag_cb(wave, sb) : 16 * cb;
                const double *Cin = g.A + g.Rb + ro + l15 + (long)(g.Cb + co + l4) * g.lda;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[cb][r] = Cin[(long)(4 * r) * g.lda];
            }
        }
        // nothing that waits for a load may move up between the loads
        __builtin_amdgcn_sched_barrier(0);
        solve16_stage_store(Fs, f6, wv);
    }
    __syncthreads(); // A
    f.load_lds(Fs);
    BQ_SSTAMP(g.stamps, 1, f.la[3][2][3] + f.wf[3][3], 0)
    // Q rows (row block by) -> LDS (eight waves: by waves 4-7, slab_upper_waves); P rows (row
    // block bx) stay in registers
    double4_t xp[4];
    if (NW == 4 && bx != by) {
        double4_t xq[4];
        solve16(tq, f, xq);
        slab_publish(Qs, wave, l15, l4, xq);
    }
    solve16(tp, f, xp);
    if (bx == by)
        slab_publish(Qs, wave, l15, l4, xp);
    BQ_SSTAMP(g.stamps, 2, xp[3][3], 0)
    // The tile was loaded raw (see the prologue) and is negated HERE: behind the solve, which has
    // given it 3,000 cycles to arrive, and in front of the stores below -- the wait counts
    // stores too, and behind them the tile's wait would drain them on workgroup 0's path.
    // (acc[3] of a diagonal tile is never read.)
    // (The pins keep the sign flips, and the wait with them, from sinking to the accumulators'
    // first uses behind the barrier.)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
        if (cb < 3 || bx != by) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double v = -acc[cb][r];
                asm volatile("" : "+v"(v));
                acc[cb][r] = v;
            }
        }
    __builtin_amdgcn_sched_barrier(0);
    // the solved rows are the factor: tile column 0 owns the write
    if (by == 0)
        solve16_store(g.A + g.Rb + 16 * wave + l15 + (long)(g.j0 + l4) * g.lda, g.lda, xp);
    __syncthreads(); // Q
    BQ_SSTAMP(g.stamps, 3, acc[1][3] + acc[0][0], 0)
    if (bx == by)
        slab_update_diag(Qs, wave, acc);
    else
        slab_update_offdiag(Qs, xp, acc);
    BQ_SSTAMP(g.stamps, 4, acc[1][3] + acc[0][0], 0)
    BQ_SSTAMP_STORES(g.stamps, 27, acc[1][3] + acc[0][0], g.swg, 0, false)
    // tile column 0 is the next panel: it goes to the scratch column (the diagonal tile,
    // which workgroup 0 factors in place, and the Schur complement of the last step stay in A)
    // (the pipelined form never comes here with a diagonal tile, and workgroup 0 is one)
    if (!(NW == 8 && PIPE) && blockIdx.x == 0 && g.factor_next) {
        // the next diagonal block never touches memory between its update and its factor
        // (only the ten lower blocks: the factor never reads a lane above its column's own)
        if constexpr (NW == 8) {
            // eight waves: the blocks go, packed, where the fragments were -- every wave has had
            // its fragments since the barrier in front of the update -- and ONE barrier later
            // the factor's waves pick their columns out of them (slab_load_blocks8)
            slab_pack_blocks8(Fs, wave, acc);
            __syncthreads(); // F
            slab_factor_next8(g, plds, (STAMP && blockIdx.z == 0) ? g.stamps + 5 : nullptr);
            BQ_SSTAMP_STORES(g.stamps, 25, 0, 0, 0, false)
            return;
        }
        // four waves: it lands where the Q rows were: every wave must be through with them
        __syncthreads(); // T
#pragma unroll
        for (int sb = 0; sb < 3; ++sb)
            if (sb < slab_diag_nb(wave)) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Ts[16 * slab_diag_rb(wave, sb) + l15 +
                       64 * (16 * slab_diag_cb(wave, sb) + l4 + 4 * r)] = -acc[sb][r];
            }
        __syncthreads(); // F
        // (col0: the global column of this sweep's first column, for the failure report)
        potf2_body<NW>(g.A + g.r0 + (long)g.r0 * g.lda, g.lda, g.col0 + g.r0, g.dout, g.info + g.b,
                       plds, Ts, 64, (STAMP && blockIdx.z == 0) ? g.stamps + 5 : nullptr,
                       g.out.scal ? g.out.scal + 4 * g.b + 1 : nullptr);
        return;
    }
    const bool to_s = by == 0 && bx > 0 && !g.last;
    double *Cout = to_s ? g.Sout + g.Rb + 16 * wave + l15 + (long)l4 * g.lds
                        : g.A + g.Rb + 16 * wave + l15 + (long)(g.Cb + l4) * g.lda;
    const long ldo = to_s ? g.lds : g.lda;
    if (bx == by) {
        slab_store_diag<TILES>(g, wave, acc);
        BQ_SSTAMP_STORES(g.stamps, 25, 0, 0, 0, true)
    } else {
        if constexpr (TILES != SLAB_TILES_EMIT) {
            const bool wt = slab_wg_wt();
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    slab_tile_store<TILES>(Cout + (long)(16 * cb + 4 * r) * ldo, -acc[cb][r], wt);
        }
        // (the last step's tiles are the Schur complement of the border: slab_emit)
        if (slab_emits<TILES>(g)) {
            const SlabOut o = g.out; // (by value: every field is read once, not per entry)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    slab_emit(o, g.b, g.Rb + 16 * wave + l15, g.Cb + 16 * cb + l4 + 4 * r,
                              -acc[cb][r]);
        }
        BQ_SSTAMP_STORES(g.stamps, 28, 0, g.swg, 0, true)
    }
}

// NW = 8 (launch_slab_step has the rule): 512 threads; in an off-diagonal tile waves 4-7 solve the
// Q rows while waves 0-3 solve the P rows; in a diagonal tile they update the tile behind the
// solve's column blocks (PIPE, below; !PIPE: they pass the update's barriers), and in workgroup 0
// they join the diagonal factor as its second wave per SIMD (potf2f_body<8>: the chain 16.5 k ->
// 13.2 k cycles).
// PIPE (BQ_DIAG_PIPE, the shipped eight-wave form; NW = 8 only): in a DIAGONAL tile waves 4-7 do
// not idle.  The tile's update is a sum over the four 16-column k-blocks of X, and k-block c needs
// only x_c, which solve16 delivers about 8 dependent MFMAs before x_{c+1}: waves 0-3 publish
// every x_c in the Q rows behind a barrier of its own (B_c), and waves 4-7, which requested the
// ten lower blocks of the C tile at entry, run k-block c of the update (12 MFMAs per wave) while
// waves 0-3 solve x_{c+1}.  Behind the solve stand only the last k-block and the hand-off.  Same
// MFMAs on the same operands in the same order per accumulator as PIPE = false, on other waves.
// STAMP: [2] is wave 0 behind B_3, [3] stays 0, [4] is wave 4 behind its last MFMA, [16..18] /
// [19..21] are wave 4's / wave 0's arrivals at B_1 .. B_3.
//
// Barriers per workgroup, in order -- every wave of a workgroup executes the same row:
//                                                        waves 0-3            waves 4-7 (NW = 8)
//   off-diagonal tile (any NW, PIPE)                     A Q                  A Q
//   diagonal, NW = 4, workgroup 0 with factor_next       A Q T F [+ factor]   --
//   diagonal, NW = 4, else (`last`, other tiles)         A Q                  --
//   diagonal, NW = 8, !PIPE, workgroup 0, factor_next    A Q F [+ factor]     A Q F [+ factor]
//   diagonal, NW = 8, !PIPE, else                        A Q                  A Q
//   diagonal, NW = 8, PIPE, workgroup 0, factor_next     A B0 B1 B2 B3 F [+]  A B0 B1 B2 B3 F [+]
//   diagonal, NW = 8, PIPE, else                         A B0 B1 B2 B3        A B0 B1 B2 B3
// A: fragments staged; Q: solved rows in LDS; T: every wave through with the Q rows; B_c: x_c in
// LDS; F: updated diagonal block in LDS; [+ factor]: the barriers of the diagonal factor
// (potf2.h), all waves alike.  `last` has factor_next = 0; workgroup 0 is a diagonal tile; which
// row a workgroup takes depends on blockIdx and kernel arguments only, never on the wave.
// TILES (SLAB_TILES_*, above; launch_slab_step has the rule; write-through with NW = 8 only): how the
// updated tiles leave; the solved rows and everything workgroup 0 stores are plain stores always.
template <bool STAMP, int NW = 4, bool PIPE = false, int TILES = SLAB_TILES_PLAIN>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void slab_step_kernel(double *__restrict__ A, long lda,
                                                        long astride,
                                                        const double *__restrict__ Sin,
                                                        double *__restrict__ Sout, long lds,
                                                        long sstride, int ntot, int j0,
                                                        const double *__restrict__ din,
                                                        double *__restrict__ dout, long dstride,
                                                        int factor_next, int last,
                                                        int *__restrict__ info, int col0,
                                                        long long *stamps, SlabOut out)
{
    static_assert(NW == 8 || TILES != SLAB_TILES_WT, "write-through: the one-round eight-wave steps");
    BQ_SSTAMP(stamps, 0, 0, 0)
    BQ_SSTAMP_STORES(stamps, 24, 0, 0, 0, false)
    // One region, 52 KiB -- a workgroup of this kernel must fit into what ONE retiring workgroup
    // of the 64-tile product frees on a CU (36 KiB + the 16 KiB four of them leave over), or it
    // starves behind a trailing update running on the other stream.  First 4096 doubles: the Q
    // rows of the tile, [k][row] (A-fragment reads are contiguous over rows); afterwards, in
    // workgroup 0, the factor's panel slots (four waves: first the updated diagonal block on its
    // way to the factor).  Behind them: the fragments of L_jj and W (BQ_SLAB_FW doubles); after
    // the update, in workgroup 0 of eight waves, the updated diagonal block as ten packed blocks.
    __shared__ __attribute__((aligned(16))) double plds[4096 + BQ_SLAB_FW];
    __builtin_amdgcn_s_setprio(3);
    const int b = blockIdx.z;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int bx, by;
    tri_decode(blockIdx.x, bx, by);
    const int r0 = j0 + 64;
    // (the last step's tiles that nobody reads: before the first barrier, the whole workgroup)
    if constexpr (TILES == SLAB_TILES_EMIT) {
        if (slab_tile_dead(out, bx, by, r0 + 64 * bx))
            return;
    }
    // (STAMP: tile (T - 1, 1) of a step with at least three tile rows)
    const int swg = STAMP && gridDim.x >= 6 ? (int)gridDim.x - (ntot - r0) / 64 + 1 : -1;
    BQ_SSTAMP_STORES(stamps, 26, 0, swg, 0, false)
    const SlabWg g = {A + (long)b * astride, Sin + (long)b * sstride, Sout + (long)b * sstride,
                      din + (long)b * dstride, dout + (long)b * dstride, lda, lds, j0, r0,
                      r0 + 64 * bx, r0 + 64 * by, bx, by, wave, b, factor_next, last, col0, swg,
                      info, stamps, out};
    // A diagonal tile of the pipelined form is a path of its own from here to its return:
    // nothing of it is shared with the off-diagonal tiles, whose code and registers stay the
    // one-phase form's.
    if constexpr (NW == 8 && PIPE) {
        if (g.bx == g.by) {
            if (g.wave >= 4) {
                slab_pipe_update<STAMP, TILES>(g, plds);
                return;
            }
            slab_pipe_solve<STAMP>(g, plds);
            return;
        }
    }
    if (NW == 8 && g.wave >= 4) {
        slab_upper_waves(g, plds);
        return;
    }
    slab_one_phase<STAMP, NW, PIPE, TILES>(g, plds);
}
#undef BQ_SSTAMP_STORES
#undef BQ_SSTAMP
#undef BQ_SSTAMP_AT

// The assembly of the bordered system with the first launch of the slab sweep folded in: the
// tiles of column block 0 also fill the sweep's scratch column, and the workgroup of tile
// (0, 0) factors the leading 64 x 64 block and with it starts the failure flag and log|K| (its
// factor stores them; the stored form, !REGS, clears them in front of it) -- one launch, one memset
// and 12 us less per pass of a small problem.
// NW = 8 (one problem or a few: the grid has a CU per workgroup): 512 threads, waves 4-7 only
// join workgroup (0, 0) (potf2f_body<8>).

// The leading 64 x 64 block computed where the factor wants it: wave w's columns 4 (NW q + w) + s
// of row `lane`, each entry by the assembly's own function (same arithmetic, same bits).  Rows and
// columns below 64 <= npad carry a point or are identity padding, never the y row.  All of a
// group's column points are requested before its first exp (all groups' where the dimension leaves
// the registers for it; wv: the wave's number as a vector value, so that they are vector loads --
// gram.h, assemble_tile), and the exps are independent.
// The strict upper triangle -- the assembly has always written it, the factor never does -- is
// stored from the registers: plain stores, nothing waits for them here.
template <int D, int NW>
__device__ __forceinline__ void first_block_regs(Potf2FT<NW> &st, const double *__restrict__ pts,
                                                 const GaussParams &gm, double *__restrict__ A,
                                                 long lda, const Layout &L, int wv, int lane)
{
    constexpr int NG = 16 / NW;
    constexpr int GQ = 4 * NG * D <= 32 ? NG : 1; // groups whose points are held at a time
    Layout L0 = L;
    L0.yrow = -1;
    GaussParams g;
    g.c = gm.c, g.s2 = gm.s2;
#pragma unroll
    for (int k = 0; k < D; ++k)
        g.nh[k] = gm.nh[k];
    const bool pi = lane < L.n;
    double xi[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        xi[k] = pts[k + (long)(pi ? lane : 0) * D];
#pragma unroll
    for (int q0 = 0; q0 < NG; q0 += GQ) {
        double xj[GQ][4][D];
#pragma unroll
        for (int q = 0; q < GQ; ++q)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int c = 4 * (NW * (q0 + q) + wv) + s;
#pragma unroll
                for (int k = 0; k < D; ++k)
                    xj[q][s][k] = pts[k + (long)(c < L.n ? c : 0) * D];
            }
        // nothing that waits for a load may move up between the loads
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < GQ; ++q)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int c = 4 * (NW * (q0 + q) + wv) + s;
                st.a[q0 + q][s] =
                    bordered_entry_flat<D>(lane, c, pi, c < L.n, xi, xj[q][s], g, L0, 0.0);
            }
    }
    // (every entry is computed before the first store: the stores sit under a branch each, and the
    // exps, sunk to their stores, were one basic block -- one dependent chain -- after the other)
#pragma unroll
    for (int q = 0; q < NG; ++q)
#pragma unroll
        for (int s = 0; s < 4; ++s)
            PIN(st.a[q][s]);
#pragma unroll
    for (int q = 0; q < NG; ++q)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int c = 4 * (NW * q + wv) + s;
            if (lane < c)
                A[lane + (long)c * lda] = st.a[q][s];
        }
}

// REGS (BQ_FIRST_REGS, the shipped form): workgroup (0, 0) assembles nothing but the leading block,
// in registers, and factors it from there (first_block_regs) -- the unfactored lower triangle never
// reaches memory: no store of it, no drain, no barrier, no reload.  Rows 64-127 of column block 0,
// the other half of its tile, are the work of workgroup (0, 2): tile (0, 2) lies strictly above
// the diagonal and has nothing else to do; at ntot = 128, where the grid has no such tile, the
// launcher adds the row (one workgroup per problem: gridDim.x = 1 there).
// !REGS: workgroup (0, 0) stores its tile, waits for the stores and loads the block back.
// STAMP: the probe's instantiation (bq_probe_first_launch): workgroup (0, 0) of problem 0 records
// s_memtime at [0] entry, [1] block assembled, [2 ..] the factor's own five (potf2.h, BQ_STAMP).
template <int D, int NW = 4, bool REGS = true, bool STAMP = false>
__global__ __launch_bounds__(64 * NW) void assemble_first_kernel(
    const double *__restrict__ pts, long pstride, const double *__restrict__ y, long ystride,
    const GaussParams *__restrict__ gp, int gpstride, double *__restrict__ A, long lda,
    long astride, Layout L, double *__restrict__ S0, long lds, long sstride,
    double *__restrict__ dinv, long dstride, int *__restrict__ info, double *__restrict__ scal,
    long long *stamps)
{
    __shared__ __attribute__((aligned(16))) double plds[BQ_POTF2_LDS_DOUBLES];
    const int b = blockIdx.z;
    const bool corner = blockIdx.x == 0 && blockIdx.y == 0;
    long long *const st0 = (STAMP && corner && b == 0) ? stamps : nullptr;
    if (st0 && threadIdx.x == 0)
        st0[0] = (long long)__builtin_amdgcn_s_memtime();
    A += (long)b * astride;
    if constexpr (REGS) {
        if (blockIdx.x == 0 && blockIdx.y == 2) {
            if (NW == 4 || threadIdx.x < 256)
                assemble_tile<D>(pts + (long)b * pstride, y + (long)b * ystride,
                                 gp[(long)b * gpstride], A, lda, L, S0 + (long)b * sstride, lds, 64,
                                 0, 128);
            return;
        }
        if (corner) {
            // info[b] = 0 and scal[4 b + 1] = 0 are not stored here: the factor is told that the
            // failure flag and log|K| start with it (potf2f_run, `fresh`) -- it reads neither and
            // stores both, a failure or none.  One writer per word, nothing to order.
            __builtin_amdgcn_s_setprio(3);
            const int lane = threadIdx.x & 63;
            Potf2FT<NW> st;
            first_block_regs<D, NW>(st, pts + (long)b * pstride, gp[(long)b * gpstride], A, lda, L,
                                    (int)(threadIdx.x >> 6), lane);
            if (st0) {
                asm volatile("" ::"v"(st.a[0][0]));
                if (threadIdx.x == 0)
                    st0[1] = st0[2] = (long long)__builtin_amdgcn_s_memtime();
            }
            potf2f_run<NW>(st, A, lda, 0, dinv + (long)b * dstride, info + b, plds,
                           st0 ? st0 + 2 : nullptr, scal ? scal + 4 * b + 1 : nullptr, L.n, true);
            return;
        }
    }
    if (NW == 4 || threadIdx.x < 256)
        assemble_tile<D>(pts + (long)b * pstride, y + (long)b * ystride, gp[(long)b * gpstride],
                         A, lda, L, S0 + (long)b * sstride, lds);
    if (!REGS && corner) {
        if (threadIdx.x == 0) {
            info[b] = 0;
            if (scal)
                scal[4 * b + 1] = 0.0; // log|K|: the factors add to it (SlabOut)
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads(); // the block's 64 x 64 entries (rows 0..63 of this tile) are in memory
        if (st0 && threadIdx.x == 0)
            st0[1] = (long long)__builtin_amdgcn_s_memtime();
        __builtin_amdgcn_s_setprio(3);
        potf2_body<NW>(A, lda, 0, dinv + (long)b * dstride, info + b, plds, nullptr, 0,
                       st0 ? st0 + 2 : nullptr, scal ? scal + 4 * b + 1 : nullptr, L.n);
    }
}

// first launch of a slab sweep: workgroup 0 factors the leading diagonal block, the others
// copy panel column 0 (rows >= 64) into the scratch column -- one launch instead of two
__global__ __launch_bounds__(256) void slab_first_kernel(double *__restrict__ A, long lda,
                                                         long astride, double *__restrict__ S,
                                                         long lds, long sstride, int ntot,
                                                         double *__restrict__ dinv, long dstride,
                                                         int *__restrict__ info, int col0)
{
    __shared__ __attribute__((aligned(16))) double plds[BQ_POTF2_LDS_DOUBLES];
    const int b = blockIdx.z;
    A += (long)b * astride;
    if (blockIdx.x == 0) {
        __builtin_amdgcn_s_setprio(3);
        potf2_body(A, lda, col0, dinv + (long)b * dstride, info + b, plds);
        return;
    }
    // 64 rows x 64 columns per workgroup: thread t copies row (t & 63) of 16 columns
    const int i = 64 * (int)blockIdx.x + (threadIdx.x & 63);
    const int jb = (threadIdx.x >> 6) * 16;
    if (i < ntot) {
        double *dst = S + (long)b * sstride + i + (long)jb * lds;
        const double *src = A + i + (long)jb * lda;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            dst[(long)j * lds] = src[(long)j * lda];
    }
}

// ---------------------------------------------------------------------------
// The same idea for the 64-column steps INSIDE a wide panel (outer block 128 / 256): one
// launch per step instead of two (left-looking slab update + fused diagonal factor, panel
// solve).  Step s of the panel that starts at column K0 (j0 = K0 + 64 s), one workgroup per
// 64-row block below the diagonal block of slab s:
//   * solve its own rows of slab s (from the scratch column Sin; the first step of a panel
//     reads them from A) and write them, the final L, to A;
//   * if the panel has a slab s + 1: solve the rows of row block s + 1 as well (every
//     workgroup for itself, through LDS) and bring its rows of slab s + 1 up to date with
//     ALL slabs 0 .. s of the panel (left-looking, k = 64 (s + 1): the earlier slabs' L from
//     A, slab s from registers / LDS); the result goes to the scratch column Sout, the input
//     of step s + 1 -- except in workgroup 0, whose rows ARE row block s + 1: its result is
//     the next diagonal block, handed through LDS to potf2_body<NW>.
// Nothing waits on another workgroup.  grid: ((ntot - j0 - 64) / 64, 1, batch); block 64 NW.
// NW = 8 (launch_panel_step has the rule): waves 4-7 solve the rows of row
// block s + 1 beside waves 0-3's solve of the workgroup's own rows, and join workgroup 0's
// diagonal factor (potf2f_body<8>); the left-looking product stays on waves 0-3, in its k order.
// ---------------------------------------------------------------------------
template <int NW = 4>
__global__ __launch_bounds__(64 * NW) void panel_step_kernel(double *__restrict__ A, long lda,
                                                         long astride,
                                                         const double *__restrict__ Sin,
                                                         double *__restrict__ Sout, long lds,
                                                         long sstride, int K0, int j0,
                                                         const double *__restrict__ din,
                                                         double *__restrict__ dout, long dstride,
                                                         int has_next, int first,
                                                         double *__restrict__ SL,
                                                         int *__restrict__ info)
{
    // 40 KiB (see slab_step_kernel): the solved Q rows, then -- workgroup 0 -- the next diagonal
    // block and the factor's slots in the same 4096 doubles
    __shared__ __attribute__((aligned(16))) double plds[BQ_POTF2_LDS_DOUBLES];
    double *const Qs = plds;
    double *const Ts = plds;
    __builtin_amdgcn_s_setprio(3);
    const int b = blockIdx.z;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    A += (long)b * astride;
    Sin += (long)b * sstride;
    Sout += (long)b * sstride;
    din += (long)b * dstride;
    dout += (long)b * dstride;
    const int r0 = j0 + 64;                 // row block s + 1 = the next diagonal block
    const int Rb = r0 + 64 * blockIdx.x;    // this workgroup's rows
    const int l15 = lane & 15, l4 = lane >> 4;
    SL += (long)b * 4096;
    // The first step of a panel reads its slab straight from A (no staging launch).  Every
    // workgroup reads its own rows before it overwrites them; the one block that others read
    // too -- row block s + 1, for their own solve -- is written by workgroup 0 to the side
    // buffer SL instead, and workgroup 0 of the NEXT step (where those rows are the diagonal
    // block's and nobody reads them) moves it into place.
    const double *Sp = first ? A + (long)j0 * lda : Sin;
    const long ldsp = first ? lda : lds;
    if (!first && j0 - K0 == 64 && blockIdx.x == 0) {
        double *dst = A + j0 + (long)(j0 - 64) * lda;
        for (int e = threadIdx.x; e < 4096; e += 64 * NW)
            dst[(e & 63) + (long)(e >> 6) * lda] = SL[e];
    }
    if (NW == 8 && wave >= 4 && (!has_next || blockIdx.x == 0)) {
        // no second row block to solve: the barriers of waves 0-3 below, in their order, and
        // workgroup 0's diagonal factor
        if (!has_next)
            return;
        __syncthreads();
        __syncthreads();
        __syncthreads();
        potf2_body<8>(A + r0 + (long)r0 * lda, lda, r0, dout, info + b, plds, Ts, 64);
        return;
    }

    Solve16Regs<> f;
    f.load_global(A + j0 + (long)j0 * lda, lda, din, l15, l4);
    double4_t xp[4];
    if (has_next && blockIdx.x != 0 && (NW == 4 || wave >= 4)) {
        const int wq = wave & 3;
        double4_t xq[4];
        double tq[4][4];
        solve16_load(Sp + r0 + 16 * wq + l15 + (long)l4 * ldsp, ldsp, tq);
        solve16(tq, f, xq);
        slab_publish(Qs, wq, l15, l4, xq);
        if (NW == 8) {
            __syncthreads(); // (the one in front of the slab-s product below)
            return;
        }
    }
    {
        double tp[4][4];
        solve16_load(Sp + Rb + 16 * wave + l15 + (long)l4 * ldsp, ldsp, tp);
        solve16(tp, f, xp);
    }
    {
        // (a lone workgroup has no readers to protect, and no next step to move the block)
        const bool side = first && has_next && blockIdx.x == 0 && gridDim.x > 1;
        double *Lw = side ? SL + 16 * wave + l15 + 64 * l4
                          : A + Rb + 16 * wave + l15 + (long)(j0 + l4) * lda;
        solve16_store(Lw, side ? 64 : lda, xp);
    }
    if (!has_next)
        return;
    if (blockIdx.x == 0)
        slab_publish(Qs, wave, l15, l4, xp);
    // my rows of slab s + 1 (columns r0 .. r0 + 63), still as the last trailing update left them
    const double *Cin = A + Rb + 16 * wave + l15 + (long)(r0 + l4) * lda;
    double4_t acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[cb][r] = -Cin[(long)(16 * cb + 4 * r) * lda];
    // slabs 0 .. s-1 of the panel: both operands from A (P: my rows, Q: row block s + 1)
    {
        const double *Pg = A + Rb + 16 * wave + l15 + (long)(K0 + l4) * lda;
        const double *Qg = A + r0 + l15 + (long)(K0 + l4) * lda;
        // 16 columns (4 k-steps) per trip, the next trip's 20 fragments in flight meanwhile
        const int kend = j0 - K0; // multiple of 64
        double pa[4], qa[4][4], pb[4], qb[4][4];
#define BQ_PANEL_LOAD(PF, QF, KK)                                                                  \
    _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                  \
    {                                                                                              \
        PF[t] = Pg[(long)((KK) + 4 * t) * lda];                                                    \
        _Pragma("unroll") for (int cb = 0; cb < 4; ++cb) QF[t][cb] =                               \
            Qg[16 * cb + (long)((KK) + 4 * t) * lda];                                              \
    }
#define BQ_PANEL_MFMA(PF, QF)                                                                      \
    _Pragma("unroll") for (int t = 0; t < 4; ++t) _Pragma("unroll") for (int cb = 0; cb < 4; ++cb) \
        acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(QF[t][cb], PF[t], acc[cb], 0, 0, 0);
        if (kend > 0) {
            BQ_PANEL_LOAD(pa, qa, 0)
            for (int kk = 0; kk < kend; kk += 32) {
                BQ_PANEL_LOAD(pb, qb, kk + 16)
                __builtin_amdgcn_sched_barrier(0);
                BQ_PANEL_MFMA(pa, qa)
                __builtin_amdgcn_sched_barrier(0);
                const int kn = kk + 32 < kend ? kk + 32 : kk; // clamped: values unused past the end
                BQ_PANEL_LOAD(pa, qa, kn)
                __builtin_amdgcn_sched_barrier(0);
                BQ_PANEL_MFMA(pb, qb)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#undef BQ_PANEL_LOAD
#undef BQ_PANEL_MFMA
    }
    __syncthreads();
    // slab s: P from registers, Q from LDS
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double pf = xp[c][r];
            const double *qrow = Qs + (16 * c + l4 + 4 * r) * 64 + l15;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(qrow[16 * cb], pf, acc[cb], 0, 0, 0);
        }
    if (blockIdx.x == 0) {
        __syncthreads(); // Ts is where the Q rows were
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Ts[16 * wave + l15 + 64 * (16 * cb + l4 + 4 * r)] = -acc[cb][r];
        __syncthreads();
        potf2_body<NW>(A + r0 + (long)r0 * lda, lda, r0, dout, info + b, plds, Ts, 64);
        return;
    }
    double *Cout = Sout + Rb + 16 * wave + l15 + (long)l4 * lds;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            Cout[(long)(16 * cb + 4 * r) * lds] = -acc[cb][r];
}

// ---------------------------------------------------------------------------
// The whole kb x kb diagonal block of an outer block factored by ONE workgroup per matrix
// (potrf.hip, enqueue_potrf_dfirst: a batch's diagonal factor D).  The one-launch steps above
// spend a chip on it -- every tile's workgroup solves the panel rows it needs itself, 253 VGPRs,
// hundreds of workgroups per step -- which is right for a chain that has the chip to itself and
// wrong for one that is supposed to hide beside the previous block's trailing update: there its
// workgroups displace the update's.  Here the factor of a matrix occupies one workgroup (eight
// waves) from its first column to its last:
//     per 64-column slab: the 64 x 64 factor (potf2f_body<8>, leaves its record behind);
//     the rows below, 16 per wave-task, on the matrix cores (solve16);
//     the trailing tiles of the block, 32 x 32 per wave-task, k = 64 (all fragments requested
//     up front), lower triangle only;
// phases separated by workgroup barriers -- the block (1.6 MB at kb = 448) lives in L2, the same
// CU wrote what it reads.  64 matrices = 64 workgroups; ~20 us per slab.
// grid (batch), block 512.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void wg_update32(double *__restrict__ C, long ldc,
                                            const double *__restrict__ P,
                                            const double *__restrict__ Q, long ldp, int row0,
                                            int col0, int lane)
{
    const int l15 = lane & 15, l4 = lane >> 4;
    double pa[16][2], qa[16][2], cold[2][2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const double *pp = P + row0 + 16 * h + l15 + (long)l4 * ldp;
        const double *qq = Q + col0 + 16 * h + l15 + (long)l4 * ldp;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            pa[ks][h] = pp[(long)(4 * ks) * ldp];
            qa[ks][h] = qq[(long)(4 * ks) * ldp];
        }
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                cold[tm][tn][rr] =
                    C[(row0 + 16 * tm + l15) + (long)(col0 + 16 * tn + l4 + 4 * rr) * ldc];
    __builtin_amdgcn_sched_barrier(0);
    double4_t acc[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
            acc[tm][tn] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 16; ++ks)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
                acc[tm][tn] =
                    __builtin_amdgcn_mfma_f64_16x16x4f64(qa[ks][tn], pa[ks][tm], acc[tm][tn], 0, 0, 0);
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            if (col0 + 16 * tn >= row0 + 16 * tm + 16)
                continue; // (wave-uniform: a 16 x 16 block above the diagonal)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                C[(row0 + 16 * tm + l15) + (long)(col0 + 16 * tn + l4 + 4 * rr) * ldc] =
                    cold[tm][tn][rr] - acc[tm][tn][rr];
        }
}

__global__ __launch_bounds__(512) void potrf_wg_kernel(double *__restrict__ A, long lda,
                                                       long astride, int kb,
                                                       double *__restrict__ rec, long rstride,
                                                       int *__restrict__ info, int col0)
{
    __shared__ __attribute__((aligned(16))) double plds[BQ_POTF2_LDS_DOUBLES];
    __builtin_amdgcn_s_setprio(3);
    const int b = blockIdx.x;
    A += (long)b * astride;
    rec += (long)b * rstride;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int ns = kb >> 6;
    for (int s = 0; s < ns; ++s) {
        double *Ass = A + 64 * s + (long)(64 * s) * lda;
        double *rs = rec + (long)s * BQ_DINV_HALF;
        potf2_body<8, true>(Ass, lda, col0 + 64 * s, rs, info + b, plds);
        // (explicit: what this workgroup stored is in memory before its other waves read it)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int nr = ns - s - 1;
        if (nr == 0)
            break;
        const int r0 = 64 * (s + 1);
        {
            Solve16Regs<> f;
            f.load_global(Ass, lda, rs, l15, l4);
            for (int task = wave; task < 4 * nr; task += 8) {
                double *Xr = A + r0 + 16 * task + l15 + (long)(64 * s + l4) * lda;
                double t[4][4];
                double4_t x[4];
                solve16_load(Xr, lda, t);
                solve16(t, f, x);
                solve16_store(Xr, lda, x);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        {
            const double *Pn = A + r0 + (long)(64 * s) * lda; // the solved panel, rows from r0
            double *Cn = A + r0 + (long)r0 * lda;
            const int ntask = 4 * (nr * (nr + 1) / 2);
            for (int task = wave; task < ntask; task += 8) {
                int ti, tj;
                tri_decode(task >> 2, ti, tj);
                const int q = task & 3;
                const int row0 = 64 * ti + 32 * (q & 1), cl0 = 64 * tj + 32 * (q >> 1);
                if (cl0 > row0)
                    continue; // the upper 32 x 32 block of a diagonal tile
                wg_update32(Cn, lda, Pn, Pn, lda, row0, cl0, lane);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}
