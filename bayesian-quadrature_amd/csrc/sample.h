// sample.h -- joint posterior samples of a resident fit: the device normals, the factor's diagonal
// and the triangular product out = mean 1^T + tril(L_c) Z (fit.hip, bq_gp_sample).
// Part of the libbqhip.so kernel set; compiled into k_reduce.hip (host.h lists the units).
//
// Determinism: a normal depends on (seed, its element index) alone, and every entry of the product
// is one accumulator that takes its k steps in ascending order -- the same order whatever the
// number of sample columns, so a column of the result does not depend on how many there are, and
// two calls give the same bits.
#pragma once
#include "common.h"

// Philox4x32-10 (Salmon et al., SC11; the Random123 constants): counter c[4], key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0, c[1] = (uint32_t)p1, c[2] = n2, c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// Z (Mp x S, ld ldz): element e = j + M s, j < M, is one standard normal by Box-Muller from one
// Philox block keyed by the seed -- the cosine branch alone, so an element's value depends on
// nothing but (seed, e); rows M .. Mp are zeros.  u1 lies in (0, 1]: the logarithm is finite.
__global__ __launch_bounds__(256) void normal_fill_kernel(double *__restrict__ Z, long ldz, int M,
                                                          int Mp, int S, uint64_t seed)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)Mp * S)
        return;
    const int j = (int)(t % Mp);
    const long s = t / Mp;
    double z = 0.0;
    if (j < M) {
        const uint64_t e = (uint64_t)j + (uint64_t)M * (uint64_t)s;
        uint32_t c[4] = {(uint32_t)e, (uint32_t)(e >> 32), 0u, 0u};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        const uint64_t a = ((uint64_t)(c[0] >> 5) << 26) + (c[1] >> 6) + 1;
        const uint64_t b = ((uint64_t)(c[2] >> 5) << 26) + (c[3] >> 6);
        const double u1 = (double)a * 0x1p-53, u2 = (double)b * 0x1p-53;
        z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
    }
    Z[j + s * ldz] = z;
}

// the diagonal of the matrix about to be factored: `add` on its first M entries, 1 on the padding
// (rows M .. Mp, whose rows and columns are zero otherwise)
__global__ __launch_bounds__(256) void sample_diag_kernel(double *__restrict__ A, long lda, int M,
                                                          int Mp, double add)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Mp)
        return;
    double *p = A + i + (long)i * lda;
    if (i >= M)
        *p = 1.0;
    else if (add != 0.0)
        *p += add;
}

constexpr int BQ_SAMPLE_LDK = 66; // k stride of a staged column of Z: conflict-free fragment reads

// out (M x S, ld ldo) = mean 1^T + tril(L) Z on v_mfma_f64_16x16x4_f64.  L: Mp x Mp, ld ldl, a
// Cholesky factor in its lower triangle -- what lies above the diagonal is not part of it (the
// factorisation leaves the matrix it was given there) and is never read: the diagonal block's
// entries with k > row are masked to zero.  Z: Mp x S, ld ldz, its rows M .. Mp zeros.
// grid (Mp / 64, ceil(S / 64)), 256 threads: workgroup (x, y) takes row block Mp / 64 - 1 - x (the
// block with the longest k loop starts first) and sample columns 64 y .. 64 y + 63; wave w its rows
// 16 w .. 16 w + 15.  Per 64-row k block, up to and including the diagonal one: the block's rows
// of Z for the chunk's columns go through LDS (column c at BQ_SAMPLE_LDK c), the wave's 16 x 64
// piece of L comes straight from memory (no other wave reads it).  The product is taken
// transposed -- tile rows = sample columns, tile columns = rows of out: register r of tile ct is
// entry (row m0 + (lane & 15), column 64 y + 16 ct + (lane >> 4) + 4 r), so the accumulators start
// as mean and a store instruction writes 16 consecutive rows.  Stores: rows < M, columns < S.
__global__ __launch_bounds__(256) void tri_sample_kernel(const double *__restrict__ L, long ldl,
                                                         const double *__restrict__ Z, long ldz,
                                                         const double *__restrict__ mean,
                                                         double *__restrict__ out, long ldo, int M,
                                                         int S)
{
    __shared__ double Zs[64 * BQ_SAMPLE_LDK];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int rb = (int)gridDim.x - 1 - (int)blockIdx.x;
    const int c0 = 64 * (int)blockIdx.y;
    const int ncol = min(64, S - c0); // live sample columns of this chunk
    const int row = 64 * rb + 16 * w + l15; // the row of L and of out this lane loads and stores
    const double mu = row < M ? mean[row] : 0.0;
    double4_t acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
        acc[ct] = double4_t{mu, mu, mu, mu};

    for (int kb = 0; kb <= rb; ++kb) {
        const bool diag = kb == rb;
        // this lane's entries of L for the block's 16 k steps, (row, 64 kb + 4 ks + l4), and its 16
        // entries of the block's rows of Z.  All 32 loads leave before the first barrier and nothing
        // is done with a value until after it: a masked entry of L is loaded from the row's
        // diagonal entry and a dead column of Z from the chunk's last live one, and both become
        // zeros by a select below -- a branch around a load, or a select right behind it, makes
        // the loads wait for one another
        double a[16], zv[16];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const int k = 64 * kb + 4 * ks + l4;
            a[ks] = L[row + (long)(diag && k > row ? row : k) * ldl];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i)
            zv[i] = Z[64 * kb + lane + (long)(c0 + min(w + 4 * i, ncol - 1)) * ldz];
        __syncthreads(); // the previous block's fragments have been read
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = w + 4 * i;
            Zs[BQ_SAMPLE_LDK * c + lane] = c < ncol ? zv[i] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const double am = diag && 64 * kb + 4 * ks + l4 > row ? 0.0 : a[ks];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                    Zs[BQ_SAMPLE_LDK * (16 * ct + l15) + 4 * ks + l4], am, acc[ct], 0, 0, 0);
        }
    }
    if (row < M) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = c0 + 16 * ct + l4 + 4 * r;
                if (col < S)
                    out[row + (long)col * ldo] = acc[ct][r];
            }
    }
}
