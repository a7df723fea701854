// solve16.h -- a wave's 16 rows of the panel solve from 16 x 16 block inverses, once
// Shared by trsm.h, slab.h (k_panel.hip) and gemm.h, trsmsweep.h (k_gemm.hip); host.h lists the units.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------
// X (16 x 64) <- T L^-T against a factored 64 x 64 block L in four 16-column block steps,
//   X_c = (T_c - sum_{b<c} X_b L_cb^T) W_cc^T,   W_cc = L_cc^-1 (the record potf2.h leaves behind),
// 40 MFMAs per wave (trsm.h has the scheme).  Solve 16 rows of the panel: returns X^T blocks x[c]
// (D / B-fragment form: x[c][r] of lane l is X[row l & 15][16 c + (l >> 4) + 4 r]); t likewise,
// raw.  The A fragments come from a provider f: f.a(c, bb, r) is L_cb's (lane l: L[16 c + (l & 15)]
// [16 bb + (l >> 4) + 4 r]), f.w(c, r) is -W_cc's (-W_c[l & 15][(l >> 4) + 4 r]); every solve of a
// wave shares them.  MFMA order per accumulator: for each earlier block bb ascending, r = 0..3 into
// acc, then r = 0..3 into x_c -- whoever compares bits between two kernels relies on it.
// Callers that act between the blocks (publish x_c, store it) call the blocks themselves.
// ---------------------------------------------------------------------------
// The lane's place in a 16 x 16 x 4 operand: row (A) / column (B, D) l15, k or D-row group l4.
// The convention for a helper here and in slab.h: one that indexes LDS or stages (load_lds*,
// solve16_stage_*, slab_store_diag, slab_pack_blocks8, the slab_update_* pair) takes the two
// from threadIdx ITSELF, through these functions -- behind a function parameter their range is
// unknown where the helper is first optimised, and hipcc then settles on other address arithmetic
// and another order of the step's loads than for the same code written in place.  One that only
// offsets a global pointer or the Q rows (load_global, slab_publish*) takes them as PARAMETERS:
// written the first way, an MFMA of panel_step_kernel<4> moved.  A new helper follows the first
// rule unless its kernel's instruction sequence says otherwise (tools/asm_compare.py; LABBOOK).
__device__ __forceinline__ int mfma_l15() { return (threadIdx.x & 63) & 15; }
__device__ __forceinline__ int mfma_l4() { return (threadIdx.x & 63) >> 4; }

template <int C, class Frags>
__device__ __forceinline__ void solve16_block(const double (&tc)[4], const Frags &f, double4_t (&x)[4])
{
    // acc = sum_b L_cb X_b^T - T_c^T
    double4_t acc = {-tc[0], -tc[1], -tc[2], -tc[3]};
#pragma unroll
    for (int bb = 0; bb < C; ++bb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.a(C, bb, r), x[bb][r], acc, 0, 0, 0);
    // X_c^T = -W_cc acc
    double4_t xc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r)
        xc = __builtin_amdgcn_mfma_f64_16x16x4f64(f.w(C, r), acc[r], xc, 0, 0, 0);
    x[C] = xc;
}

template <class Frags>
__device__ __forceinline__ void solve16(const double (&t)[4][4], const Frags &f, double4_t (&x)[4])
{
    solve16_block<0>(t[0], f, x);
    solve16_block<1>(t[1], f, x);
    solve16_block<2>(t[2], f, x);
    solve16_block<3>(t[3], f, x);
}

// t[c][r] = S[row][16 c + 4 r] of a pointer that already carries the lane's row and l4 columns
__device__ __forceinline__ void solve16_load(const double *__restrict__ S, long lds, double (&t)[4][4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            t[c][r] = S[(long)(16 * c + 4 * r) * lds];
}

// ... and the way back: block C of the solved rows / all four, to a pointer of the same kind
template <int C>
__device__ __forceinline__ void solve16_store_block(double *X, long ldx, const double4_t (&x)[4])
{
#pragma unroll
    for (int r = 0; r < 4; ++r)
        X[(long)(16 * C + 4 * r) * ldx] = x[C][r];
}

__device__ __forceinline__ void solve16_store(double *X, long ldx, const double4_t (&x)[4])
{
    solve16_store_block<0>(X, ldx, x);
    solve16_store_block<1>(X, ldx, x);
    solve16_store_block<2>(X, ldx, x);
    solve16_store_block<3>(X, ldx, x);
}

// The LDS staging area of a one-launch step: the six 16 x 16 blocks (c, bb), c > bb, below L_jj's
// diagonal at 256 ((c (c - 1)) / 2 + bb), element (i, k) at i + 16 k, then the four NEGATED block
// inverses as they lie in the record.  BQ_SLAB_FW doubles.
#define BQ_SLAB_FW (10 * 256)
__device__ __forceinline__ constexpr int solve16_lds_l(int c, int bb) { return 256 * ((c * (c - 1)) / 2 + bb); }
__device__ __forceinline__ constexpr int solve16_lds_w(int c) { return 256 * (6 + c); }

// Staged by 256 threads, ten doubles each, in two halves: the caller issues its other global loads
// and its sched_barrier(0) between request() and store() -- nothing that waits for a load may move
// up between the loads.  L11: L_jj's origin; rec: the block's record (64 reciprocal pivots first).
__device__ __forceinline__ void solve16_stage_request(const double *L11, long ldl, const double *rec,
                                                      double (&f)[6], double (&wv)[4])
{
    const int t = threadIdx.x;
    const double *Lt = L11 + (t & 15) + (long)(t >> 4) * ldl;
#pragma unroll
    for (int c = 1; c < 4; ++c)
#pragma unroll
        for (int bb = 0; bb < c; ++bb)
            f[(c * (c - 1)) / 2 + bb] = Lt[16 * c + (long)(16 * bb) * ldl];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        wv[q] = rec[64 + 256 * q + t];
}

__device__ __forceinline__ void solve16_stage_store(double *Fs, const double (&f)[6],
                                                    const double (&wv)[4])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 6; ++q)
        Fs[256 * q + t] = f[q];
    double *Ws = Fs + solve16_lds_w(0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        Ws[256 * q + t] = -wv[q];
}

// Provider 1: the fragments resident in registers, 64 per lane; loaded once per wave from global
// memory or, per column block, from the staging area.  wf holds -W_cc; with NEG_AT_USE, W_cc as
// loaded, negated in front of its MFMA (trsm_blk_kernel: hipcc schedules the two forms differently).
template <bool NEG_AT_USE = false> struct Solve16Regs {
    double la[4][3][4], wf[4][4];
    __device__ __forceinline__ double a(int c, int bb, int r) const { return la[c][bb][r]; }
    __device__ __forceinline__ double w(int c, int r) const { return NEG_AT_USE ? -wf[c][r] : wf[c][r]; }
    // L11: the factored block's origin; rec: its record.  W_c[l15][l4 + 4 r] at 256 c + 64 r.
    __device__ __forceinline__ void load_global(const double *__restrict__ L11, long ldl,
                                                const double *__restrict__ rec, int l15, int l4)
    {
        const double *Ll = L11 + l15 + (long)l4 * ldl;
        const double *W = rec + 64 + l15 + 16 * l4;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                wf[c][r] = NEG_AT_USE ? W[256 * c + 64 * r] : -W[256 * c + 64 * r];
#pragma unroll
        for (int c = 1; c < 4; ++c)
#pragma unroll
            for (int bb = 0; bb < c; ++bb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    la[c][bb][r] = Ll[16 * c + (long)(16 * bb + 4 * r) * ldl];
    }
    // The lane's fragment in the staging area (which holds the inverses negated): -W_c's relative
    // to the first W block, L_cb's relative to Fs.  Both loaders below read through these.
    static __device__ __forceinline__ int lds_w_at(int c, int r) { return 256 * c + 64 * r + mfma_l15() + 16 * mfma_l4(); }
    static __device__ __forceinline__ int lds_l_at(int c, int bb, int r)
    {
        return solve16_lds_l(c, bb) + mfma_l15() + 16 * (mfma_l4() + 4 * r);
    }
    template <int C> __device__ __forceinline__ void load_lds_block(const double *Fs)
    {
        static_assert(!NEG_AT_USE, "the staging area holds -W");
        const double *Ws = Fs + solve16_lds_w(0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            wf[C][r] = Ws[lds_w_at(C, r)];
#pragma unroll
        for (int bb = 0; bb < C; ++bb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                la[C][bb][r] = Fs[lds_l_at(C, bb, r)];
    }
    // All four blocks, every W in front of the first L: the order of the one-phase step's LDS
    // reads (four load_lds_block calls give that kernel another schedule).
    __device__ __forceinline__ void load_lds(const double *Fs)
    {
        static_assert(!NEG_AT_USE, "the staging area holds -W");
        const double *Ws = Fs + solve16_lds_w(0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                wf[c][r] = Ws[lds_w_at(c, r)];
#pragma unroll
        for (int c = 1; c < 4; ++c)
#pragma unroll
            for (int bb = 0; bb < c; ++bb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    la[c][bb][r] = Fs[lds_l_at(c, bb, r)];
    }
};

// Provider 2: every fragment read from global memory where its MFMA uses it -- the form of the
// k_gemm.hip kernels, which sit at 128 VGPRs for four workgroups per CU and have no room for 64
// resident fragments.  L11 / rec as above.
struct Solve16Stream {
    const double *Ll, *W;
    long ldl;
    __device__ __forceinline__ Solve16Stream(const double *__restrict__ L11, long ldl_,
                                             const double *__restrict__ rec)
        : Ll(L11 + mfma_l15() + (long)mfma_l4() * ldl_), W(rec + 64 + mfma_l15() + 16 * mfma_l4()),
          ldl(ldl_)
    {
    }
    __device__ __forceinline__ double a(int c, int bb, int r) const
    {
        return Ll[16 * c + (long)(16 * bb + 4 * r) * ldl];
    }
    __device__ __forceinline__ double w(int c, int r) const { return -W[256 * c + 64 * r]; }
};

// Block C of a wave's rows out of a column-major 64 x 64 tile in LDS (Tw: the lane's row, column
// l4), solved and stored at once -- the epilogue of the fused product and of the one-launch sweep.
template <int C, class Frags>
__device__ __forceinline__ void solve16_tile_block(const double *Tw, const Frags &f,
                                                   double4_t (&x)[4], double *Xr, long ldx)
{
    const double tc[4] = {Tw[64 * (16 * C)], Tw[64 * (16 * C + 4)], Tw[64 * (16 * C + 8)],
                          Tw[64 * (16 * C + 12)]};
    solve16_block<C>(tc, f, x);
    solve16_store_block<C>(Xr, ldx, x);
}

template <class Frags>
__device__ __forceinline__ void solve16_tile(const double *Tw, const Frags &f, double *Xr, long ldx)
{
    double4_t x[4];
    solve16_tile_block<0>(Tw, f, x, Xr, ldx);
    solve16_tile_block<1>(Tw, f, x, Xr, ldx);
    solve16_tile_block<2>(Tw, f, x, Xr, ldx);
    solve16_tile_block<3>(Tw, f, x, Xr, ldx);
}
