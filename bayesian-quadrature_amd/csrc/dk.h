// dk.h -- the derivative operand D_k = K0 o u_k, u_k = r_k^2 / w_k^3 - 1 / w_k, of a resident fit,
// generated from its points and never stored: what the log-ML gradient (gemm.h), the Hessian
// (hess.h) and the posterior's derivatives in the hyper-parameters (ptheta.h) share.
//
//   gauss_k0<D>        K0(i, j) and the r_k^2 of one pair of points
//   dk_weight          u_k from r_k^2
//   dka_sums<D>        a row of the vectors D_k a, k < D
// hess_prod_kernel and ptheta_quad_kernel call the first two from their own copies of the chunk
// loop: with the loop, or its generated-operand block alone, in a function here both compile to
// other registers, spills and occupancy than they had (LABBOOK).
// Every expression here is the one its callers' results are defined by, bit for bit: hipcc
// contracts multiply-adds by the shape of an expression, so none of them may be rearranged.
#pragma once
#include "common.h"

#define BQ_DK_KC 16 // k columns per chunk of the MFMA products over D_k

// K0(i, j) and r_k^2 from the points, gauss_q's arithmetic
template <int D>
__device__ __forceinline__ double gauss_k0(const double (&xi)[D], const double *__restrict__ xj,
                                           const GaussParams &g, double (&r2)[D])
{
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double t = xi[k] - xj[k];
        r2[k] = t * t;
        q += r2[k] * g.nh[k];
    }
    return g.c * exp_gauss(q);
}

// u_k = r_k^2 / w_k^3 - 1 / w_k from iw = 1 / w_k, iw2 = iw^2 and r2 = r_k^2
__device__ __forceinline__ double dk_weight(double iw, double iw2, double r2)
{
    return (iw2 * r2 - 1.0) * iw;
}

// sum[k] = (D_k a)_i, k < D, in each of the 16 lanes jl that share row i (zeros for i >= n): lane jl
// adds the columns jl, jl + 16 .. below n in order, then a shuffle tree.  Whole waves call it.
template <int D>
__device__ __forceinline__ void dka_sums(const HessJob &hj, int i, int jl, double (&sum)[D])
{
#pragma unroll
    for (int k = 0; k < D; ++k)
        sum[k] = 0.0;
    if (i < hj.n) {
        double xi[D], iw[D], iw2[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            xi[k] = hj.pts[k + (long)i * D];
            iw[k] = hj.iw[k];
            iw2[k] = iw[k] * iw[k];
        }
        for (int j = jl; j < hj.n; j += 16) {
            double r2[D];
            const double ka = gauss_k0<D>(xi, hj.pts + (long)j * D, hj.g, r2) * hj.alpha[j];
#pragma unroll
            for (int k = 0; k < D; ++k)
                sum[k] += ka * dk_weight(iw[k], iw2[k], r2[k]);
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < D; ++k)
            sum[k] += __shfl_xor(sum[k], off);
}
