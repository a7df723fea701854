// types.h -- plain structs and constants shared by the kernels and the host side of
// libbqhip.so (no device code: every translation unit includes it).
#pragma once
#include <stdint.h>

#define BQ_MAXD 8

// Per-problem scratch of the 64-column panel step: 64 reciprocal pivots of the current
// diagonal block, then the inverses of its four 16 x 16 diagonal sub-blocks (column-major,
// 256 doubles each) -- written by potf2f_body, read by trsm_blk_kernel.
#define BQ_DINV_HALF (64 + 4 * 256)
// two halves: the one-launch slab step (slab.h) writes the next block's half while this
// block's is still being read
#define BQ_DINV_STRIDE (2 * BQ_DINV_HALF)

// Gaussian kernel parameters of one batch element:
//   k(p,q) = c * exp( sum_k nh[k] (p_k - q_k)^2 ),  c = h^2 / prod(sqrt(2 pi) w_k),
//   nh[k] = -1 / (2 w_k^2);  s2 = s^2 is added on the diagonal of Kxx.
struct GaussParams {
    double c;
    double s2;
    double nh[BQ_MAXD];
};

// Layout of one bordered system (gram.h: assemble_kernel has the picture)
struct Layout {
    int n, npad, M, yrow, ntot; // yrow < 0: no y row
};

// A product C -= P Q^T whose C has not been written yet (round 6): instead of loading its tile of
// C the kernel computes the tile's entries of the bordered system -- assemble_tile's values, bit
// for bit -- from the problem's points.  r, c: the global row / column of C(0, 0) in that system.
struct GramSeed {
    const double *pts; // d x ntot per problem
    long pstride;
    const double *y;
    long ystride;
    const GaussParams *gp;
    int gpstride;
    Layout L;
    int d, r, c;
};

// The log-ML gradient's product (gemm.h, gemm_lds_grad_kernel): the tile of G = alpha alpha^T -
// Kxx^-1 is reduced against the kernel's derivatives instead of being stored.  part: d + 2 partial
// sums per workgroup.
struct GradJob {
    const double *alpha; // npad
    const double *pts;   // d x n
    double *part;
    GaussParams g;
    int n;
};

// the scalings of the gradient's d + 2 sums (fold_kernel<GradScale>, wgsum.h)
struct GradScale {
    double f[BQ_MAXD + 2];
};

// The log-ML Hessian (hess.h): what its kernels read of the fit
struct HessJob {
    const double *pts;   // d x n
    const double *alpha; // npad
    GaussParams g;
    double iw[BQ_MAXD];  // 1 / w_k
    int n, npad;
};

// rows of the matrix that holds a fit's solved vectors u, z_1 .. z_d (ptheta.h; d + 1 <= 9 of them
// are used): one 64-row block, the fewest the row sweeps take
#define BQ_PTHETA_ROWS 64

// The polynomial trend of a fit (trend.h).  The basis: degree 0 .. 2 over t = (x - c) / rho, p
// columns -- 1; t_1 .. t_d; t_k t_l (k <= l, k outer) -- at most 45 at d = BQ_MAXD.
struct TrendBasis {
    int degree, p;
    double c[BQ_MAXD], rho[BQ_MAXD];
};
constexpr int trend_p(int degree, int d)
{
    return degree == 0 ? 1 : degree == 1 ? 1 + d : 1 + d + d * (d + 1) / 2;
}
// rows of the matrix that holds G = L^-1 H as rows (one 64-row block, like BQ_PTHETA_ROWS)
#define BQ_TREND_ROWS 64
#define BQ_TREND_MAXP 45
// the largest p whose sums v.G_k ride in the row reductions' pass over V (rowdot_trend_kernel)
#define BQ_TREND_ONEPASS_MAXP 8
// what trend_solve_kernel leaves on the device, in doubles: the status (0: A factored), log|A|,
// b^T beta | beta (64, zero from p on) | A^-1 (p x p, ld p) -- so far the head that goes back to
// the host -- | L_A (p x p, ld p, zero above its diagonal)
#define BQ_TREND_STATUS 0
#define BQ_TREND_LOGDET 1
#define BQ_TREND_BTB 2
#define BQ_TREND_BETA 8
#define BQ_TREND_AINV (BQ_TREND_BETA + BQ_TREND_ROWS)
#define BQ_TREND_HEAD (BQ_TREND_AINV + 2048)
#define BQ_TREND_LA BQ_TREND_HEAD
#define BQ_TREND_STATE (BQ_TREND_LA + 2048)

// the sums' places (D = d): [G sums | trace sums | quadratic terms]
//   G:     S_K, S_k (d), S_kl (k <= l, row by row), S_ss
//   trace: sum C o C, sum C o Ki, sum Ki o Ki, sum C o B_k (d), sum Ki o B_k (d), sum B_k o B_l^T (k <= l)
//   quad:  (D_p a)^T Ki (D_q a), p <= q over the d + 2 parameters, row by row
constexpr int hess_npair(int d) { return d * (d + 1) / 2; }
constexpr int hess_ng(int d) { return 2 + d + hess_npair(d); }
constexpr int hess_nt(int d) { return 3 + 2 * d + hess_npair(d); }
constexpr int hess_nq(int d) { return hess_npair(d + 2); }
// place of the pair (k, l), k <= l < d, in a row-by-row upper triangle
constexpr int hess_pair(int d, int k, int l)
{
    return k * d - k * (k - 1) / 2 + (l - k);
}

// Growing a resident fit by k observations (append.h): what append_commit_kernel reads and writes.
struct AppendJob {
    // side buffers
    const double *V;    // kp x npad (ld kp): the swept rows
    const double *S;    // kp x kp (ld kp): L_S in its lower triangle
    const double *zn;   // z_new[i] at zn[i * zstride]
    long zstride;
    const double *xn;   // d x k new points
    const double *yn;   // k new targets
    const int *info;    // 0: every pivot of S was positive
    // the fit (after growth: the new buffers)
    double *A;
    long ldl;
    double *pts, *y, *dinv;
    double *out;        // [info | - | logml, logdet, qf]: the words a (re)fit reads back
    double logdet, qf;  // of the n old points
    int d, n, k, kp, yrow;
};

// The pivoted partial Cholesky of a posterior (pivchol.h): what a step's kernels read instead of
// asking the host -- the current pivot and its gain, and whether the factorisation has ended.
struct PivcholState {
    int done, rank, p, pad;
    double gain;
};

// Square-root-warped quadrature of a fit (sqwarp.h): what sq_xform_kernel reads of the measure.
// A point x becomes t = [a1 x | a2 (x - m2)] (a1, a2: D x D, row-major; the second half only for
// the pair sums that take sums of coordinates), and, where the weight carries the density of a
// Gaussian form, exp(klogc - |kl (x - km)|^2 / 2) times its weight (kl lower triangular).
template <int D>
struct SqXform {
    double a1[D * D], a2[D * D], m2[D];
    double kl[D * D], km[D], klogc;
};
// ... and the same for every d, as the host computes it from (h, w, mu, Sigma) (moments.hip,
// sq_forms): the two transforms with the constants in front of their pair sums,
//   W(p, q) = cw exp(-|t1(p) - t1(q)|^2 / 2 - |t2(p) + t2(q)|^2 / 2),
//   Q_ij    = cq n_i n_j exp(-|tq(x_i) - tq(x_j)|^2 / 2),  n = exp(klogc - |kl (x - mu)|^2 / 2)
struct SqForms {
    double a1w[BQ_MAXD * BQ_MAXD], a2w[BQ_MAXD * BQ_MAXD], cw;
    double a1q[BQ_MAXD * BQ_MAXD], kl[BQ_MAXD * BQ_MAXD], klogc, cq;
    double mu[BQ_MAXD];
};
// the pair sums' tile: columns staged through LDS at a time, and the granule of a column slice;
// rows per workgroup; the most slices
#define BQ_SQ_TJ 128
#define BQ_SQ_RB 256
#define BQ_SQ_MAX_SLICES 64

// Removing k observations from a resident fit (remove.h): what remove_compact_kernel reads of the
// old fit and writes into buffers of the new layout.
#define BQ_REMOVE_M_DOUBLES (128 * 128) // the 128 x 128 transform of one block column (scratch)
struct RemoveJob {
    // the old fit
    const double *A;    // bordered factor, z in row yrow
    long ldl;
    int yrow;
    const double *pts, *y;
    // ascending old indices: the n2 survivors, the k removed
    const int *keep, *rem;
    // buffers of the layout of n2 points
    double *A2;         // ntot2 x ntot2
    long ldl2;
    double *pts2, *y2;  // d x ntot2, npad2
    double *V;          // ntot2 x kp (ld ntot2): L[keep, rem], z[rem] in row npad2
    int d, n2, npad2, ntot2, k, kp;
};

// Read-out of a bordered system folded into the one-launch sweep (slab.h): the diagonal factors
// add their share of log|K| to scal[4b + 1] as they go, and the LAST step's tiles -- the Schur
// complement of the border -- store what finalize_kernel would read from it (no launch of its own).
struct SlabOut {
    double *scal, *mean, *var; // scal: 4 per problem {logml, logdet, qf, -}; mean / var: mstride per problem
    long mstride;
    int n, npad, M, yrow;
};

// batched active-sampling systems (moments.h: assemble_esm_kernel)
struct EsmLayout {
    int ns, nsc, npad, ntot; // points [0, nsc] (nsc+1 of them), border rows npad, npad+1
};

// closed-form Gaussian integrals (moments.h): exp(logc - |linv (p - mu)|^2 / 2)
template <int D>
struct GaussForm {
    double mu[D];        // subtracted from the point(s) to form z
    double linv[D * D];  // row-major lower-triangular inverse Cholesky factor
    double logc;         // -(D log 2pi + log|C|) / 2
};

// the uniform measure on a box (moments.h, int_K_box_kernel): per axis the two ends and, from the
// host, 1 / (sqrt2 w) and 1 / (hi - lo)
template <int D>
struct BoxForm {
    double lo[D], hi[D], rw[D], rl[D];
};

// one job of rows_step_kernel (gemm.h)
struct RowsJob {
    double *C;
    long ldc;
    const double *P1, *Q1, *P2, *Q2;
    long ldp1, qsj1, qsk1, ldp2, qsj2, qsk2;
    int k1, k2;
    int ny;    // tile columns of this job
    int write; // 1: C = -(products); 0: C -= products
};
