// potf2.h -- the 64x64 diagonal Cholesky block (four or eight waves) and the record it leaves behind
// Part of the libbqhip.so kernel set; compiled into k_gemm.hip / k_panel.hip / probe.hip (host.h lists the units).
#pragma once
#include "common.h"

// ===========================================================================
// 64 x 64 diagonal Cholesky block by NW = 4 waves (one per SIMD) or 8 (two per SIMD).  Every wave
// holds all 64 rows (lane = row) and 16 / NW four-column panels: the matrix is cut into sixteen
// 4-column panels dealt round-robin to the waves, panel P to wave P % NW.  Panel P is factored by
// its owner (in-panel updates by v_readlane) and published to its LDS slot (a full block keeps all
// sixteen -- the epilogue reads the factor out of them --, a padded one a ring of three); after ONE
// workgroup barrier per panel every wave applies the rank-4 update to its own later columns.
// What the factor leaves behind, for its own panel solve and for every sweep over the factor:
// the factored block in memory and its RECORD, BQ_DINV_HALF doubles -- 64 reciprocal pivots
// (potf2f_rcp), then the inverses W_b of the four 16 x 16 diagonal sub-blocks, each stored whole and
// column-major (W_b[r][k] at 64 + 256 b + r + 16 k, the strict upper triangle exact zeros: solve16.h
// multiplies by the whole block).  ONE function, potf2f_block_inverse, computes W_b for every
// producer of a record -- both epilogues of potf2f_run and diag_winv_kernel (trsm.h) --, so two
// records of the same factor agree in every bit.
// What was measured on gfx950 and shaped this file (tools/potf2_probe.py, tools/c2_timeline.py):
//   * a wave's time per panel is set by the waves that only update in the early panels
//     (64 FMAs + 36 LDS reads, ~1100 cycles when every group waited for its own reads) and by
//     the owner's path (own-panel update + four pivots, ~740 cycles) in the late ones -- not
//     by the instruction count of the pivot: Newton vs Halley, per-pivot selects or not,
//     moved the 15,000-cycle chain by 2 %;
//   * published-column counters polled in LDS instead of barriers (every panel its own slot,
//     the next owner applying columns as they appear) were SLOWER: 24,500 cycles;
//   * the epilogue after the last pivot: 5,800 cycles as row dot products (41 LDS waits), 2,900 as
//     four VALU slices of forward substitution, 1,400 on the four-block MFMA (LABBOOK, "Diagonal
//     factor: block inverses on the four-block MFMA");
//   * a launch cannot end before the factor's stores have drained, and the next launch reads the
//     factor first: with the short epilogue the write-back has to START before the chain ends
//     (Potf2FSteps, steps 12-14), or the launch gets longer although workgroup 0 is through sooner.
// ===========================================================================
// NW waves (4, or 8: two per SIMD -- potf2f_body): panel P = columns 4P .. 4P + 3 belongs to wave
// P % NW, which holds it as its group P / NW
template <int NW> struct Potf2FT {
    double a[16 / NW][4]; // a[g][s] = column 4 (NW g + w) + s of row `lane`
};
using Potf2F = Potf2FT<4>;

// LDS of the factor: the panels' slots (4 x 64 doubles each: sixteen, or a ring of three) in the first 4096
// doubles -- the region may hold the factor's own input block, which every wave has in
// registers before the first panel is published --, then the four 16 x 16 diagonal
// sub-blocks (1024 doubles)
#define BQ_POTF2F_SLOTS (16 * 256)
#define BQ_POTF2F_LDS_DOUBLES (BQ_POTF2F_SLOTS + 1024)

// Factor panel P (columns 4P .. 4P+3, group QP = P >> 2) held by this wave and publish it.
// The dependent chain of a pivot, in instruction hops (an fp64 hop costs 12-16 cycles):
//   readlane d -> rsq y0 -> {t = d y0, l0 = a y0} -> e = 1 - t y0 -> {p = 1/2 + 3/8 e, m = l0 e}
//   -> l = l0 + m p -> dn = a' - l l (the next pivot's diagonal, in its own lane) -> readlane.
// The scaled column is formed directly (l = a y1 = l0 + l0 e p, a third-order step from the
// v_rsq_f64 seed: error 5 e^3 / 16 ~ 1e-21 for the 2^-24 seed measured on gfx950), never the
// refined reciprocal, and the next diagonal entry needs no broadcast: every lane squares its
// own l.  The pivot row is scaled like every other row (L_cc = d r, about an ulp from sqrt d):
// no per-pivot selects, no failure bookkeeping -- a non-positive pivot makes r NaN or infinite
// and everything after it NaN, and potf2f_body finds it afterwards as the first NaN on the
// diagonal.
template <int P, int NW = 4>
__device__ __forceinline__ void potf2f_factor(Potf2FT<NW> &st, double *slot, int lane)
{
    constexpr int QP = P / NW;
    double dn = st.a[QP][0];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int c = 4 * P + s;
        const double d = readlane_f64(dn, c);
        const double y0 = __builtin_amdgcn_rsq(d);
        const double t = d * y0;
        const double l0 = st.a[QP][s] * y0;
        const double e = __builtin_fma(-t, y0, 1.0);
        const double p = __builtin_fma(0.375, e, 0.5);
        const double m = l0 * e;
        const double l = __builtin_fma(m, p, l0);
        if (s < 3)
            dn = __builtin_fma(-l, l, st.a[QP][s + 1]);
#pragma unroll
        for (int s2 = s + 1; s2 < 4; ++s2)
            st.a[QP][s2] = __builtin_fma(-l, readlane_f64(l, 4 * P + s2), st.a[QP][s2]);
        st.a[QP][s] = l;
        slot[s * 64 + lane] = l;
    }
}

// Rank-4 update of this wave's columns of the groups in QMASK by the panel in `slot` (li: the
// panel's entries in this lane's row).  All multipliers of all groups are requested before
// the first FMA (uniform ds_read_b128, two columns each): one LDS latency per call instead
// of one per group -- the waves that only update were the slow ones of the early panels.
template <int QMASK, int NW = 4>
__device__ __forceinline__ void potf2f_update(Potf2FT<NW> &st, const double *slot,
                                              const double (&li)[4], int w)
{
    constexpr int NG = 16 / NW;
    double2_t lk[NG][4][2];
#pragma unroll
    for (int q = 0; q < NG; ++q)
        if (QMASK & (1 << q)) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double2_t *src =
                    reinterpret_cast<const double2_t *>(slot + s * 64 + 4 * (NW * q + w));
                lk[q][s][0] = src[0];
                lk[q][s][1] = src[1];
            }
        }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < NG; ++q)
            if (QMASK & (1 << q)) {
                st.a[q][0] = __builtin_fma(-li[s], lk[q][s][0][0], st.a[q][0]);
                st.a[q][1] = __builtin_fma(-li[s], lk[q][s][0][1], st.a[q][1]);
                st.a[q][2] = __builtin_fma(-li[s], lk[q][s][1][0], st.a[q][2]);
                st.a[q][3] = __builtin_fma(-li[s], lk[q][s][1][1], st.a[q][3]);
            }
#pragma unroll
    for (int q = 0; q < NG; ++q)
        if (QMASK & (1 << q)) {
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
                PIN(st.a[q][cc]);
        }
}

// groups after Q of NG: bits Q+1 .. NG-1
#define BQ_LATER(Q, NG) (((1 << (NG)) - 1) & ~((1 << ((Q) + 1)) - 1))

// ---------------------------------------------------------------------------
// The epilogue of a full block's factor (tools/potf2_probe.py, potf2_waves.py).
// After the last pivot the factor used to copy the four 16 x 16 diagonal sub-blocks to LDS, pass a
// barrier, and run the reciprocal pivots and the four block inverses beside the write-back: 6,000
// cycles behind a chain of 13,000, most of them the inverses -- sixteen dependent steps, each lane
// of a 16-lane group running the same 120 FMAs as the other three groups' lanes.  Now:
//   * every panel keeps a slot of its own in LDS (16 x 256 doubles -- the region is there; the ring
//     of three was all the chain needs), so nothing is copied and no barrier follows the chain;
//   * wave b < 4 inverts sub-block b on the four-block MFMA (potf2f_block_inverse below): the four
//     4 x 4 diagonal inverses on the VALU, then six dependent 4 x 4 x 4 products;
//   * waves 4-7 write the factor home out of the slots; wave 4 also takes the reciprocal pivots and
//     the failure report, wave 5 log|K|.
// Measured and dropped: forward substitution in four VALU slices of four steps (sixteen dependent
// steps and five LDS / ds_bpermute round trips per sub-block, 2,900 cycles), and the same slices
// INSIDE the chain, on the waves that have run out of columns (wave w from step 8 + w on; they
// reach every later barrier ~500 cycles before the panel's owner).  Whatever those waves did --
// slices of 2, 3 or 4 steps, SIMD-aware placement, lower priority, no global stores before the
// last barrier -- stretched the owners' steps by 150-300 cycles each: the chain grew from 13,700
// to 15,500-16,500 cycles and the slab step gained 0.14 us where the factor alone gained 1.0.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double potf2f_rcp(double dg)
{
    // 1 / L_cc: v_rcp_f64 + two Newton steps (the IEEE division sequence is three times as long)
    double rc = __builtin_amdgcn_rcp(dg);
    rc = __builtin_fma(__builtin_fma(-dg, rc, 1.0), rc, rc);
    rc = __builtin_fma(__builtin_fma(-dg, rc, 1.0), rc, rc);
    return rc;
}

// Where a 16 x 16 diagonal sub-block lies: at(r, k) = L[r][k] of the sub-block.
// Sub-block b of a full block's factor in the panels' slots: column k is column k % 4 of panel
// 4 b + k / 4, rows 16 b .. 16 b + 15.
struct Potf2fInSlots {
    const double *base;
    __device__ __forceinline__ Potf2fInSlots(const double *slots, int b) : base(slots + 1040 * b) {}
    __device__ __forceinline__ double operator()(int r, int k) const { return base[64 * k + r]; }
};
// ... and one that lies on its own, column-major with leading dimension 16
struct Potf2fInBlk {
    const double *base;
    __device__ __forceinline__ explicit Potf2fInBlk(const double *blk) : base(blk) {}
    __device__ __forceinline__ double operator()(int r, int k) const { return base[16 * k + r]; }
};

// value of lane K of every quad of four lanes
template <int K>
__device__ __forceinline__ double potf2f_quad_bcast(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, 0x55 * K, 0xf, 0xf, true); // quad_perm:[K,K,K,K]
    hi = __builtin_amdgcn_mov_dpp(hi, 0x55 * K, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// column c of the inverse of a lower-triangular 4 x 4 block (l[r][k], r > k; rc[k] = 1 / l[k][k]) by
// forward substitution of the unit vector e_c; the entries above the diagonal come out as exact zeros
__device__ __forceinline__ void potf2f_inv4_column(const double (&l)[4][4], const double (&rc)[4],
                                                   int c, double (&w)[4])
{
    w[0] = (c == 0 ? 1.0 : 0.0) * rc[0];
    w[1] = __builtin_fma(-l[1][0], w[0], c == 1 ? 1.0 : 0.0) * rc[1];
    double t = __builtin_fma(-l[2][0], w[0], c == 2 ? 1.0 : 0.0);
    w[2] = __builtin_fma(-l[2][1], w[1], t) * rc[2];
    t = __builtin_fma(-l[3][0], w[0], c == 3 ? 1.0 : 0.0);
    t = __builtin_fma(-l[3][1], w[1], t);
    w[3] = __builtin_fma(-l[3][2], w[2], t) * rc[3];
}

// W = L^-1 of one lower-triangular 16 x 16 sub-block by one wave, cut into 4 x 4 blocks:
//   W_ii = L_ii^-1,   W_ij = -(sum_{j<k<=i} W_ik L_kj) W_jj   (i > j, from W L = I),
// block sub-diagonal after block sub-diagonal on v_mfma_f64_4x4x4_4b_f64 (A lane = i + 4 blk + 16 k,
// B lane = j + 4 blk + 16 k, D lane = j + 4 blk + 16 i; LABBOOK "Which fp64 MFMA").  The products
// run on transposes, W_ij^T = -W_jj^T (sum_k L_kj^T W_ik^T), so that
//   * slot blk = s of every instruction works on block ROW s of W: a level's independent products
//     share one instruction (three on the first block sub-diagonal, two on the second, one on the
//     third; the slots in front of them compute on wrapped-around operands and are thrown away);
//   * a product's D register is the next product's B operand as it stands, no relayout;
//   * lane p + 4 s + 16 q ends up with W[4 s + p][4 j + q]: a quad of lanes stores four consecutive
//     doubles of the record, which is column-major (W[r][k] at r + 16 k, solve16.h reads it so).
// The diagonal inverses are computed on the VALU twice, once as B operand (W_ss^T, slot s) and once
// as A operand (W_ss^T again; row_ror moves it to the slots s + 1 .. s + 3 that multiply by it):
// every lane substitutes the unit column it needs (four steps) and keeps its row.  Their
// reciprocal pivots: potf2f_rcp of the quad's four pivots, one per lane, spread by quad_perm.
// The depth: one LDS latency, rcp, four substitution steps, six dependent products.
// The strict upper triangle of W is stored as exact zeros (solve16_block multiplies by the whole
// block).  A NaN pivot (a failed factor) makes this sub-block's W NaN and touches no other's:
// every sub-block is its own wave's.  Every producer of a record calls THIS function on the same
// values, so that two records of one factor agree in every bit.
template <class At>
__device__ __forceinline__ void potf2f_block_inverse(const At &at, double *__restrict__ Wb, int lane)
{
    const int p = lane & 3, s = (lane >> 2) & 3, q = lane >> 4;
    // L_ss below its diagonal (the same for the sixteen lanes of slot s) and this lane's pivot
    double l[4][4];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = k + 1; r < 4; ++r)
            l[r][k] = at(4 * s + r, 4 * s + k);
    const double dg = at(4 * s + p, 4 * s + p);
    // A operands L_kj^T of the products: LT(a, c) holds in slot s the block (s - a, s - c) of L,
    // lane i + 4 s + 16 k its element [k][i]; block indices wrap in the slots nobody reads
    double lt[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = a + 1; c < 4; ++c)
            lt[a][c] = at((4 * (s - a) + q) & 15, (4 * (s - c) + p) & 15);
    const double rp = potf2f_rcp(dg);
    const double rc[4] = {potf2f_quad_bcast<0>(rp), potf2f_quad_bcast<1>(rp),
                          potf2f_quad_bcast<2>(rp), potf2f_quad_bcast<3>(rp)};
    // W_ss^T as B operand: lane j + 4 s + 16 k holds W_ss^T[k][j] = W_ss[p][q]
    // W_ss^T as A operand: lane i + 4 s + 16 k holds W_ss^T[i][k] = W_ss[q][p]
    double wq[4], wp[4];
    potf2f_inv4_column(l, rc, q, wq);
    potf2f_inv4_column(l, rc, p, wp);
    const double u0 = p == 0 ? wq[0] : p == 1 ? wq[1] : p == 2 ? wq[2] : wq[3];
    const double nwa = -(q == 0 ? wp[0] : q == 1 ? wp[1] : q == 2 ? wp[2] : wp[3]);
    // u_m: slot s holds W_{s, s-m}^T (D layout: lane p + 4 s + 16 q = W_{s, s-m}[p][q])
    const double t1 = __builtin_amdgcn_mfma_f64_4x4x4f64(lt[0][1], u0, 0.0, 0, 0, 0);
    const double t2a = __builtin_amdgcn_mfma_f64_4x4x4f64(lt[0][2], u0, 0.0, 0, 0, 0);
    const double t3a = __builtin_amdgcn_mfma_f64_4x4x4f64(lt[0][3], u0, 0.0, 0, 0, 0);
    const double u1 = __builtin_amdgcn_mfma_f64_4x4x4f64(row_ror_quads<1>(nwa), t1, 0.0, 0, 0, 0);
    const double t2 = __builtin_amdgcn_mfma_f64_4x4x4f64(lt[1][2], u1, t2a, 0, 0, 0);
    const double t3b = __builtin_amdgcn_mfma_f64_4x4x4f64(lt[1][3], u1, t3a, 0, 0, 0);
    const double u2 = __builtin_amdgcn_mfma_f64_4x4x4f64(row_ror_quads<2>(nwa), t2, 0.0, 0, 0, 0);
    const double t3 = __builtin_amdgcn_mfma_f64_4x4x4f64(lt[2][3], u2, t3b, 0, 0, 0);
    const double u3 = __builtin_amdgcn_mfma_f64_4x4x4f64(row_ror_quads<3>(nwa), t3, 0.0, 0, 0, 0);
    // block (s, s - m) of W, or zeros into the block (s, s - m + 4) above the diagonal
    double *Wl = Wb + 4 * s + p + 16 * q;
    Wl[64 * s] = u0;
    Wl[64 * ((s - 1) & 3)] = s >= 1 ? u1 : 0.0;
    Wl[64 * ((s - 2) & 3)] = s >= 2 ? u2 : 0.0;
    Wl[64 * ((s - 3) & 3)] = s >= 3 ? u3 : 0.0;
}

// sum over the wave, the same value in every lane: DPP row_shr within the rows of 16, the four row
// sums by v_readlane (a __shfl_down tree is six LDS round trips for a double)
__device__ __forceinline__ double potf2f_wave_sum(double v)
{
#define BQ_DPP_ADD(CTRL)                                                                           \
    {                                                                                              \
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);    \
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);    \
        v += __hiloint2double(hi, lo);                                                             \
    }
    BQ_DPP_ADD(0x111) // row_shr:1
    BQ_DPP_ADD(0x112)
    BQ_DPP_ADD(0x114)
    BQ_DPP_ADD(0x118)
#undef BQ_DPP_ADD
    return (readlane_f64(v, 15) + readlane_f64(v, 31)) + (readlane_f64(v, 47) + readlane_f64(v, 63));
}

// Step P, entered with panel P factored by its owner (wave P & 3) and on its way to slot
// P % 3 of the ring (EARLY: slot P); ONE workgroup barrier per panel:
//   * the owner of panel P + 1 brings only that panel up to date, runs its pivot chain and
//     publishes; what its later groups owe panel P waits until step P + 1;
//   * the owner of panel P pays that debt for panel P - 1 (slot (P - 1) % 3 is not reused
//     before step P + 1) and applies its own panel P to its later groups;
//   * the other two waves apply panel P to everything of theirs that lies behind it.
// wst (profiling probe only): every wave's arrival at and release from barrier P.
template <int P, int NW = 4, bool PAD = false, bool EARLY = false>
struct Potf2FSteps {
    // PAD, nreal: the block's rows / columns from nreal on are identity padding (a system whose
    // size is not a multiple of 64): panels that lie wholly in it are neither factored nor applied
    // -- they are what they will be -- and the sweep over the panels ends with the last real one.
    // (An instantiation of its own: the tests cost the full block's straight-line code 0.9 us.)
    // wb, ldw (eight waves, a full block; else null): where the factor goes home.  Waves 0-3 own
    // no panel behind panel 11 and have nothing left to update from step 12 on: in steps 12-14 they
    // write the 48 columns of sub-blocks 0-2 (final since panel 11 was published) out of the slots,
    // four columns per wave and step, so that these stores have drained when the launch ends.
    static __device__ __forceinline__ void run(Potf2FT<NW> &st, double *slots, int w, int lane,
                                               long long *wst, int nreal, double *wb = nullptr,
                                               long ldw = 0)
    {
        constexpr int NG = 16 / NW;
        constexpr int QP = P / NW, WP = P % NW;
        constexpr int PN = P < 15 ? P + 1 : 15, QN = PN / NW, WN = PN % NW;
        constexpr int LATER = BQ_LATER(QP, NG);
        // (EARLY: every panel keeps a slot of its own)
        const double *slot = slots + (EARLY ? P : P % 3) * 256;
        // (eight waves: arrivals only, wst[8 P + w])
        if (wst && lane == 0)
            wst[NW == 8 ? 8 * P + w : (NW * P + w) * 2] = (long long)__builtin_amdgcn_s_memtime();
        __syncthreads(); // panel P is published
        if (NW == 4 && wst && lane == 0)
            wst[(NW * P + w) * 2 + 1] = (long long)__builtin_amdgcn_s_memtime();
        double li[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
            li[s] = slot[s * 64 + lane];
        if (P < 15 && w == WN) {
            if (!PAD || 4 * PN < nreal) {
                potf2f_update<(1 << QN), NW>(st, slot, li, w);
                potf2f_factor<PN, NW>(st, slots + (EARLY ? PN : PN % 3) * 256, lane);
            }
        } else if (w == WP) {
            if (P >= 1 && LATER != 0) {
                const double *prev = slots + (EARLY ? P - 1 : (P + 2) % 3) * 256;
                double lp[4];
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    lp[s] = prev[s * 64 + lane];
                potf2f_update<LATER, NW>(st, prev, lp, w);
            }
            potf2f_update<LATER, NW>(st, slot, li, w);
        } else if (w > WP) {
            potf2f_update<(1 << QP) | LATER, NW>(st, slot, li, w);
        } else {
            potf2f_update<LATER, NW>(st, slot, li, w);
        }
        if (NW == 8 && EARLY && !PAD && P >= 12 && P <= 14 && w < 4) {
            const int c0 = 12 * w + 4 * (P - 12);
            const double *ps = slots + 64 * c0 + lane; // column c: panel c / 4, its column c % 4
            double *pw = wb + lane + (long)c0 * ldw;
            double col[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                col[c] = ps[64 * c];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (lane >= c0 + c)
                    pw[(long)c * ldw] = col[c];
        }
        if (!PAD || 4 * (P + 1) < nreal)
            Potf2FSteps<P + 1, NW, PAD, EARLY>::run(st, slots, w, lane, wst, nreal, wb, ldw);
    }
};
template <int NW, bool PAD, bool EARLY>
struct Potf2FSteps<16, NW, PAD, EARLY> {
    static __device__ __forceinline__ void run(Potf2FT<NW> &, double *, int, int, long long *, int,
                                               double *, long)
    {
    }
};

#define BQ_STAMP(k)                                                                                \
    if (stamps && threadIdx.x == 0)                                                                \
    stamps[k] = (long long)__builtin_amdgcn_s_memtime()

// The factor of a block that is already in the waves' registers (st: this wave's columns, row
// `lane`, as potf2f_body loads them).  Nothing of the block is read from `lds` or from memory;
// a caller that staged it in the slots' LDS has passed a barrier behind the last wave's load.
// fresh: this factor is the first of its sweep (the assembly's leading block,
// assemble_first_kernel): *logdet and the failure flag START here.  The factor reads neither, takes
// both as zero and stores both whatever they come to -- nobody has to clear them in front of it,
// and no wait or barrier has to order such a store against its reads.
// LATE: see the epilogue (potrf_wg_kernel, where registers are short).
template <int NW = 4, bool LATE = false>
__device__ __forceinline__ void potf2f_run(Potf2FT<NW> &st, double *__restrict__ Ab, long lda,
                                           int j0, double *__restrict__ dinv_b,
                                           int *__restrict__ info_b, double *lds,
                                           long long *stamps = nullptr, double *logdet = nullptr,
                                           int nreal = 64, bool fresh = false)
{
    constexpr int NG = 16 / NW;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double *slots = lds;
    double *blk = lds + BQ_POTF2F_SLOTS;
    BQ_STAMP(1);
    if (w == 0)
        potf2f_factor<0, NW>(st, slots, lane);
    // (per-wave barrier stamps: the four-wave probe only, and only when it asks for them with
    // stamps[5] != 0 -- they cost the chain 2,500 cycles)
    // (only the assembly's first factor passes nreal -- a system of fewer than 64 points has no
    // other --: inside slab_step_kernel the second instantiation cost C2 0.4 us per step)
    if (nreal >= 64) {
        // (a full block: the epilogue straight out of the panels' slots)
        const double ld0 = (logdet && !fresh) ? *logdet : 0.0; // one writer per launch, launches in order
        Potf2FSteps<0, NW, false, true>::run(
            st, slots, w, lane,
            (stamps && stamps[5] != 0) ? stamps + 8 : nullptr, 64, NW == 8 ? Ab : nullptr, lda);
        BQ_STAMP(2);
        BQ_STAMP(3);
        // The factor goes home.  Eight waves: columns 0-47 went in steps 12-14 (Potf2FSteps); waves
        // 0-3 go straight to the inverses and waves 4-7 write four of the last sixteen columns each
        // out of the panels' slots; four waves: every wave its own columns out of its registers
        // (the stores drain under the inverses).
        if (NW == 8 && w >= 4) {
            const int c0 = 48 + 4 * (w - 4);
            double *pw = Ab + lane + (long)c0 * lda;
            const double *ps = slots + 64 * c0 + lane; // column c: panel c / 4, its column c % 4
            asm volatile("" : "+v"(pw));
            double col[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                col[c] = ps[64 * c];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (lane >= c0 + c)
                    pw[(long)c * lda] = col[c];
        }
        if (NW == 4) {
            double *pw = Ab + lane + (long)(4 * w) * lda;
            asm volatile("" : "+v"(pw));
#pragma unroll
            for (int q = 0; q < NG; ++q) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (lane >= 4 * (NW * q + w) + s)
                        pw[(long)s * lda] = st.a[q][s];
                pw += 4 * NW * lda;
            }
        }
        // reciprocal pivots + failure report and log|K|: waves 4 and 5 of eight, else 1 and 2
        constexpr int WR = NW == 8 ? 4 : 1, WL = NW == 8 ? 5 : 2;
        // (LATE: the inverse's lane arithmetic starts HERE.  The compiler computes it in front of the
        // chain and keeps it across it; where registers are short -- potrf_wg_kernel -- it came
        // back from scratch memory right in front of the first product.  Elsewhere keeping it is
        // the faster form: with it C2 gained 0.0086 ms per step on the parent, without it 0.0095.)
        if (w < 4) {
            int il = lane;
            if (LATE)
                asm volatile("" : "+v"(il));
            potf2f_block_inverse(Potf2fInSlots(slots, w), dinv_b + 64 + 256 * w, il);
        }
        if (w == WR) {
            const double dg = slots[256 * (lane >> 2) + 64 * (lane & 3) + lane];
            dinv_b[lane] = potf2f_rcp(dg);
            const unsigned long long badm = __ballot(!(dg > 0.0) || !(dg < 1.7e308));
            if (lane == 0 && fresh)
                info_b[0] = badm != 0ull ? j0 + __builtin_ctzll(badm) + 1 : 0;
            else if (lane == 0 && badm != 0ull && info_b[0] == 0)
                info_b[0] = j0 + __builtin_ctzll(badm) + 1;
        }
        if (w == WL && logdet) {
            const double lg = potf2f_wave_sum(log(slots[256 * (lane >> 2) + 64 * (lane & 3) + lane]));
            if (lane == 0)
                *logdet = ld0 + 2.0 * lg;
        }
        BQ_STAMP(4);
        return;
    }
    // (a block of fewer than 64 real columns: the padded steps, then the epilogue below)
    Potf2FSteps<0, NW, true>::run(st, slots, w, lane, nullptr, nreal > 0 ? nreal : 1);
    BQ_STAMP(2);
    // the four 16 x 16 diagonal sub-blocks into LDS from registers:
    // blk[b][i + 16 k] = L[16 b + i][16 b + k]; my columns c = 4 (NW q + w) + sc: block c >> 4
    {
        const int bq = lane >> 4, i16 = lane & 15;
#pragma unroll
        for (int q = 0; q < NG; ++q)
#pragma unroll
            for (int sc = 0; sc < 4; ++sc) {
                const int c = 4 * (NW * q + w) + sc;
                if (bq == (c >> 4))
                    blk[256 * (c >> 4) + i16 + 16 * (c & 15)] = st.a[q][sc];
            }
    }
    __syncthreads();
    BQ_STAMP(3);
    // write back the lower triangle of my columns (the stores drain under the inverses)
    {
        double *pw = Ab + lane + (long)(4 * w) * lda;
        asm volatile("" : "+v"(pw));
#pragma unroll
        for (int q = 0; q < NG; ++q) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (lane >= 4 * (NW * q + w) + s)
                    pw[(long)s * lda] = st.a[q][s];
            pw += 4 * NW * lda;
        }
    }
    // This block's share of log|K| = 2 sum log L_cc (SlabOut: the read-out rides in the sweep;
    // one writer per launch, launches in order) -- an fp64 log is ~400 cycles of one wave: with
    // eight waves wave 4 takes it while waves 0-3 run the inverses, with four it waits until
    // wave 3 is through with its inverse (BQ_POTF2F_LOGDET below)
#define BQ_POTF2F_LOGDET                                                                           \
    {                                                                                              \
        double lg = log(blk[256 * (lane >> 4) + 17 * (lane & 15)]);                                \
        _Pragma("unroll") for (int off = 32; off > 0; off >>= 1) lg += __shfl_down(lg, off, 64);   \
        if (lane == 0)                                                                             \
            *logdet = (fresh ? 0.0 : *logdet) + 2.0 * lg;                                          \
    }
    if (NW > 4 && w >= 4) {
        if (logdet && w == 4)
            BQ_POTF2F_LOGDET
        return; // (no barrier follows: the reciprocals and the four inverses are waves 0-3's)
    }
    // reciprocal pivots (lane = column) and the failure report: a non-positive pivot left a
    // NaN on the diagonal at its own column and at every later one
    if (w == 0) {
        const double dg = blk[256 * (lane >> 4) + 17 * (lane & 15)];
        dinv_b[lane] = potf2f_rcp(dg);
        const unsigned long long badm = __ballot(!(dg > 0.0) || !(dg < 1.7e308));
        if (lane == 0 && fresh)
            info_b[0] = badm != 0ull ? j0 + __builtin_ctzll(badm) + 1 : 0;
        else if (lane == 0 && badm != 0ull && info_b[0] == 0)
            info_b[0] = j0 + __builtin_ctzll(badm) + 1;
    }
    // wave w inverts sub-block w as the full block's epilogue does, out of its copy in blk
    potf2f_block_inverse(Potf2fInBlk(blk + 256 * w), dinv_b + 64 + 256 * w, lane);
    if (NW == 4 && logdet && w == 3)
        BQ_POTF2F_LOGDET
#undef BQ_POTF2F_LOGDET
    BQ_STAMP(4);
}

// lds: BQ_POTF2F_LDS_DOUBLES doubles.  src (leading dimension lsrc): where the block is read
// from when it is not in place; when src lies in the slots' LDS (the four-wave slab step's Ts),
// pass src_in_slots so that nobody publishes before every wave has its columns.
// NW = 8: the workgroup has EIGHT waves (512 threads), two per SIMD, two panels each: the waves
// that only update have half the columns to bring up to date per panel (32 FMAs + 20 LDS reads
// instead of 64 + 36), which is what paces the early panels.
template <int NW = 4, bool LATE = false>
__device__ __forceinline__ void potf2f_body(double *__restrict__ Ab, long lda, int j0,
                                            double *__restrict__ dinv_b,
                                            int *__restrict__ info_b, double *lds,
                                            const double *src = nullptr, long lsrc = 0,
                                            bool src_in_slots = false,
                                            long long *stamps = nullptr,
                                            double *logdet = nullptr, int nreal = 64)
{
    constexpr int NG = 16 / NW;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    BQ_STAMP(0);
    Potf2FT<NW> st;
#pragma unroll
    for (int q = 0; q < NG; ++q)
#pragma unroll
        for (int s = 0; s < 4; ++s)
            st.a[q][s] = src ? src[lane + (long)(4 * (NW * q + w) + s) * lsrc]
                             : Ab[lane + (long)(4 * (NW * q + w) + s) * lda];
    if (src_in_slots)
        __syncthreads(); // the ring overwrites the block: every wave has its columns first
    potf2f_run<NW, LATE>(st, Ab, lda, j0, dinv_b, info_b, lds, stamps, logdet, nreal);
}
#undef BQ_STAMP

// ---------------------------------------------------------------------------
// The diagonal factor as every fused kernel calls it.  lds: BQ_POTF2_LDS_DOUBLES doubles; src
// (leading dimension lsrc) is where the block is read from when it is not in place -- the
// one-launch steps hand it over in the first 4096 doubles of `lds` itself.
// ---------------------------------------------------------------------------
#define BQ_POTF2_LDS_DOUBLES BQ_POTF2F_LDS_DOUBLES

template <int NW = 4, bool LATE = false>
__device__ __forceinline__ void potf2_body(double *__restrict__ Ab, long lda, int j0,
                                           double *__restrict__ dinv_b, int *__restrict__ info_b,
                                           double *lds, const double *src = nullptr,
                                           long lsrc = 0, long long *stamps = nullptr,
                                           double *logdet = nullptr, int nreal = 64)
{
    potf2f_body<NW, LATE>(Ab, lda, j0, dinv_b, info_b, lds, src, lsrc, src == lds, stamps, logdet,
                    nreal);
}
