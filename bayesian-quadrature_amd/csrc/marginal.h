// marginal.h -- the marginal of a fit: J(q) = int f(q, t) pi(q, t) dt over the integrated axes I,
// as a function of the kept axes S (include/bqhip.h, bq_gp_marginal, has the contract).
// Part of the libbqhip.so kernel set; compiled into moments.hip (host.h lists the units).
//
// J is linear in f, so it is a posterior call whose cross-Gram rows are partial kernel means
// c(q, x_j) and whose prior covariance is P(q, q').  Both kinds of measure are one expression,
//     c(q, x_j) = mult(q) [kappa_I(x_j)] exp(lp(q) + logc - |le (x_j - m(q))|^2 / 2),
// over all D axes with the host's matrices embedded at the axes' own indices (a sub-matrix of a
// lower triangle on an ascending subset of the axes is a lower triangle), zero elsewhere:
//   Gaussian  lp(q) = log pi_S(q) through ls, the inverse factor of Sigma_SS; m(q) = q on S and
//             mu_I + B (q - mu_S) on I (bm); le = diag(1 / w_S) and the inverse factor of
//             W_I + Sigma_c; mult = h^2; no column factor.  One exponent, one exp: no product of
//             three densities underflows on its own.
//   box       lp = 0; m(q) = q on S; le = diag(1 / w_S), zero on I; mult = 1[q in box_S] / vol_S;
//             the column factor kappa_box,I(x_j), h^2 included, comes from int_K_box_kernel
//             (moments.h) once per point, with the kept axes' ends at -inf and +inf, where its
//             factor is exactly 1.
// The prior is P(q, q') = scale rvol(q) rvol(q') exp(logc + lp(q) + lp(q') - |g (zq - zq')|^2 / 2)
// with zq = q - mu on S, 0 on I, and g = [diag(1 / w_S); (W_I + 2 Sigma_c)^-1/2 B] (Gaussian) or
// diag(1 / w_S) (box, scale = kk_box,I).
#pragma once
#include "common.h"

// (the forms of one call, from the host: moments.hip, marginal_plan)
template <int D>
struct MargForm {
    double mu[D], lo[D], hi[D]; // lo, hi: the box's ends on S; -inf, +inf elsewhere and for a Gaussian
    double ls[D * D];           // row-major lower triangles
    double bm[D * D];           // rows I, columns S
    double le[D * D];
    double lq, logc, scale;
    unsigned keep; // bit k: axis k is kept
};

template <int D>
struct MargPrior {
    double mu[D], lo[D], hi[D];
    double ls[D * D];
    double g[D * D];
    double lq, logc, scale, rvol;
    unsigned keep;
};

// What depends on a query point alone: qk = q and zq = q - mu on the kept axes, 0 on the others
// (whose coordinates are not read), in = q lies in the closed box, and lp = lq - |ls zq|^2 / 2.
template <int D, class F>
__device__ __forceinline__ double marg_point(const F &f, const double *__restrict__ xq, long i,
                                             double (&qk)[D], double (&zq)[D], bool &in)
{
    in = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const bool kept = (f.keep >> k) & 1u;
        const double v = kept ? xq[k + i * D] : 0.0;
        qk[k] = v;
        zq[k] = kept ? v - f.mu[k] : 0.0;
        in = in && v >= f.lo[k] && v <= f.hi[k];
    }
    double maha = 0.0;
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double y = 0.0;
#pragma unroll
        for (int c = 0; c <= r; ++c)
            y = __builtin_fma(f.ls[r * D + c], zq[c], y);
        maha = __builtin_fma(y, y, maha);
    }
    return __builtin_fma(-0.5, maha, f.lq);
}

// m(q): q on the kept axes, mu_I + B (q - mu_S) on the integrated ones
template <int D>
__device__ __forceinline__ void marg_centre(const MargForm<D> &f, const double (&qk)[D],
                                            const double (&zq)[D], double (&m)[D])
{
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double s = ((f.keep >> r) & 1u) ? qk[r] : f.mu[r];
#pragma unroll
        for (int c = 0; c < D; ++c)
            s = __builtin_fma(f.bm[r * D + c], zq[c], s);
        m[r] = s;
    }
}

// exp(lp - |le (xj - m)|^2 / 2): one entry without its factors (lp carries logc)
template <int D>
__device__ __forceinline__ double marg_entry(const MargForm<D> &f, const double (&m)[D], double lp,
                                             const double *xj)
{
    double z[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        z[k] = xj[k] - m[k];
    double maha = 0.0;
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double y = 0.0;
#pragma unroll
        for (int c = 0; c <= r; ++c)
            y = __builtin_fma(f.le[r * D + c], z[c], y);
        maha = __builtin_fma(y, y, maha);
    }
    return exp_gauss(__builtin_fma(-0.5, maha, lp));
}

// The right-hand sides of a marginal's forward sweep, K (Mp x npad, ld ldk; multiples of 64) with
// K[i, j] = c(q_i, x_j) and zeros in rows >= M and columns >= n: gram_cross_pad_kernel's shape --
// a 64 x 64 tile per 256 threads, one thread to a query row and sixteen columns, the column points
// (and, BOX, their factors colv) requested in batches of eight, clamped at the end so that no load
// sits under a branch, before the first exp.  xq: d x M, only the kept axes' rows are read.
// grid (Mp / 64, npad / 64).
template <int D, bool BOX>
__global__ __launch_bounds__(256) void marginal_cross_kernel(const double *__restrict__ xq, int M,
                                                             const double *__restrict__ x, int n,
                                                             MargForm<D> f,
                                                             const double *__restrict__ colv,
                                                             double *__restrict__ K, long ldk)
{
    const int t = threadIdx.x;
    const int i = blockIdx.x * 64 + (t & 63);
    const int jbase = blockIdx.y * 64 + (t >> 6) * 16;
    const bool row = i < M;
    double qk[D], zq[D], m[D];
    bool in;
    const double lp = marg_point<D>(f, xq, min(i, M - 1), qk, zq, in) + f.logc;
    marg_centre<D>(f, qk, zq, m);
    const bool live = row && in;
#pragma unroll
    for (int h8 = 0; h8 < 16; h8 += 8) {
        double xj[8][D], cv[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int j = min(jbase + h8 + jj, n - 1);
#pragma unroll
            for (int k = 0; k < D; ++k)
                xj[jj][k] = x[k + (long)j * D];
            cv[jj] = BOX ? colv[j] : 1.0;
        }
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int j = jbase + h8 + jj;
            double e = f.scale * marg_entry<D>(f, m, lp, xj[jj]);
            if (BOX)
                e *= cv[jj];
            K[i + (long)j * ldk] = (live && j < n) ? e : 0.0;
        }
    }
}

// mean_i = sum_j c(q_i, x_j) alpha_j without a matrix: predict_mean_kernel's pattern, one wave per
// query point, lanes striding over j, the entries' arithmetic that of marginal_cross_kernel (the
// row's factor is applied to the sum).  grid ceil(M / 4).
template <int D, bool BOX>
__global__ __launch_bounds__(256) void marginal_mean_kernel(const double *__restrict__ xq, int M,
                                                            const double *__restrict__ x, int n,
                                                            MargForm<D> f,
                                                            const double *__restrict__ colv,
                                                            const double *__restrict__ alpha,
                                                            double *__restrict__ mean)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + wave;
    if (i >= M)
        return;
    double qk[D], zq[D], m[D];
    bool in;
    const double lp = marg_point<D>(f, xq, i, qk, zq, in) + f.logc;
    marg_centre<D>(f, qk, zq, m);
    double s = 0.0;
    for (int j = lane; j < n; j += 64) {
        double xj[D];
#pragma unroll
        for (int k = 0; k < D; ++k)
            xj[k] = x[k + (long)j * D];
        double e = marg_entry<D>(f, m, lp, xj);
        if (BOX)
            e *= colv[j];
        s += e * alpha[j];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        s += __shfl_down(s, off, 64);
    if (lane == 0)
        mean[i] = in ? f.scale * s : 0.0;
}

// one entry of the prior: symmetric in its two points bit for bit (the sum of the two lp and the
// product of the two factors commute, the difference enters through squares)
template <int D>
__device__ __forceinline__ double marg_prior_entry(const MargPrior<D> &f, const double (&za)[D],
                                                   const double (&zb)[D], double lpa, double lpb,
                                                   double ra, double rb)
{
    double dz[D];
#pragma unroll
    for (int k = 0; k < D; ++k)
        dz[k] = za[k] - zb[k];
    double maha = 0.0;
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double y = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c)
            y = __builtin_fma(f.g[r * D + c], dz[c], y);
        maha = __builtin_fma(y, y, maha);
    }
    return f.scale * (ra * rb) * exp_gauss(__builtin_fma(-0.5, maha, f.logc + (lpa + lpb)));
}

// The prior covariance of a marginal at the query points: P (Mp x Mp, ld ldp, zeros in rows and
// columns >= M) -- the seed of the posterior covariance's product, in marginal_cross_kernel's
// decomposition, grid (Mp / 64, Mp / 64) -- and / or its diagonal P(q_i, q_i) (diag, M entries;
// accum: added to what is there, the read-out of var = P(q, q) - |v|^2), by the workgroups of the
// first tile column, grid (Mp / 64, 1) without P.
template <int D>
__global__ __launch_bounds__(256) void marginal_prior_kernel(const double *__restrict__ xq, int M,
                                                             MargPrior<D> f, double *__restrict__ P,
                                                             long ldp, double *__restrict__ diag,
                                                             int accum)
{
    const int t = threadIdx.x;
    const int i = blockIdx.x * 64 + (t & 63);
    const int jbase = blockIdx.y * 64 + (t >> 6) * 16;
    const bool row = i < M;
    double qk[D], zi[D];
    bool in;
    const double lpi = marg_point<D>(f, xq, min(i, M - 1), qk, zi, in);
    const double ri = in ? f.rvol : 0.0;
    if (diag && blockIdx.y == 0 && t < 64 && row) {
        const double v = marg_prior_entry<D>(f, zi, zi, lpi, lpi, ri, ri);
        diag[i] = accum ? diag[i] + v : v;
    }
    if (!P)
        return;
    for (int jj = 0; jj < 16; ++jj) {
        const int j = jbase + jj;
        double qj[D], zj[D];
        bool inj;
        const double lpj = marg_point<D>(f, xq, min(j, M - 1), qj, zj, inj);
        const double v = marg_prior_entry<D>(f, zi, zj, lpi, lpj, ri, inj ? f.rvol : 0.0);
        P[i + (long)j * ldp] = (row && j < M) ? v : 0.0;
    }
}
