// k_hess.hip -- the log-ML Hessian's kernels (hess.h) and their launcher.
#include "host.h"
#include "hess.h"

namespace bqh {

// device workspace of one Hessian beside Ki: [B_1 .. B_d | V | Z | partials | sums]
static size_t hess_tiles(int npad) { return (size_t)(npad / 64) * (size_t)(npad / 64); }
static size_t hess_off_v(int npad, int d) { return (size_t)d * npad * npad; }
static size_t hess_off_part(int npad, int d) { return hess_off_v(npad, d) + 2 * (size_t)(d + 2) * npad; }
static size_t hess_off_sums(int npad, int d)
{
    return hess_off_part(npad, d) + hess_tiles(npad) * (size_t)std::max(hess_ng(d), hess_nt(d));
}
size_t hess_ws_doubles(int npad, int d)
{
    return hess_off_sums(npad, d) + (size_t)(hess_ng(d) + hess_nt(d) + hess_nq(d));
}

// Workgroup tile of the products: the tall 256 x 64 tile where the gradient's product takes its
// 128 x 128 tile (as many workgroups), else 64 x 64
static bool hess_tall(const bq_ctx *c, int npad) { return grad_tile(c, npad) == 128; }

template <int D>
static void hess_launch_prod(bq_ctx *c, bool tall, double *C, const double *A, const double *Q,
                             const HessJob &hj, int kdim)
{
    const unsigned gy = (unsigned)hj.npad / 64;
    if (tall)
        hipLaunchKernelGGL((hess_prod_kernel<D, 4, 1, 4, 4>), dim3((unsigned)(hj.npad + 255) / 256, gy),
                           dim3(256), 0, c->stream, C, A, Q, hj, kdim);
    else
        hipLaunchKernelGGL((hess_prod_kernel<D, 2, 2, 2, 2>), dim3(gy, gy), dim3(256), 0, c->stream,
                           C, A, Q, hj, kdim);
}

template <int D>
static int hess_run(bq_ctx *c, const double *Y, double *Ki, double *ws, const HessJob &hj,
                    const double *y, double h, double s)
{
    const int npad = hj.npad, n = hj.n;
    const bool tall = hess_tall(c, npad);
    double *B = ws, *V = ws + hess_off_v(npad, D), *Z = V + (size_t)(D + 2) * npad;
    double *part = ws + hess_off_part(npad, D), *sums = ws + hess_off_sums(npad, D);
    const double n3 = (double)npad * npad * npad;
    {
        Bracket br(c, BQ_K_GEMM, n3 * 2.0 / 3.0);
        hess_launch_prod<0>(c, tall, Ki, Y, Y, hj, 0);
        HIPCHK(c, hipGetLastError());
    }
    for (int k = 0; k < D; ++k) {
        Bracket br(c, BQ_K_GEMM, 2.0 * n3);
        hess_launch_prod<D>(c, tall, B + (size_t)k * npad * npad, Ki, nullptr, hj, k);
        HIPCHK(c, hipGetLastError());
    }
    Bracket br(c, BQ_K_REDUCE);
    const unsigned g64 = (unsigned)npad / 64;
    const int nwg = (int)(g64 * g64);
    hipLaunchKernelGGL(hess_gsum_kernel<D>, dim3(g64, g64), dim3(256), 0, c->stream, Ki, hj, part);
    hipLaunchKernelGGL(hess_finalize_kernel, dim3(hess_ng(D)), dim3(256), 0, c->stream, part, nwg,
                       sums);
    hipLaunchKernelGGL(hess_trace_kernel<D>, dim3(g64, g64), dim3(256), 0, c->stream, Ki, B, hj,
                       part);
    hipLaunchKernelGGL(hess_finalize_kernel, dim3(hess_nt(D)), dim3(256), 0, c->stream, part, nwg,
                       sums + hess_ng(D));
    hipLaunchKernelGGL(hess_dka_kernel<D>, dim3((unsigned)npad / 16), dim3(256), 0, c->stream, hj, y,
                       2.0 / h, 2.0 * s, V);
    hipLaunchKernelGGL(hess_kiv_kernel, dim3((unsigned)npad / 4), dim3(256), 0, c->stream, Ki, n,
                       npad, D + 2, V, Z);
    hipLaunchKernelGGL(hess_quad_kernel, dim3(1), dim3(256), 0, c->stream, V, Z, n, npad, D + 2,
                       sums + hess_ng(D) + hess_nt(D));
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// The sums of one Hessian (types.h: hess_ng + hess_nt + hess_nq of them, at *sums inside ws) from
// Y = L^-T (npad x npad, zero below its diagonal) and the fit's alpha.  Ki: npad^2 doubles, left
// holding Kxx^-1; ws: hess_ws_doubles(npad, d).
int launch_logml_hess(bq_ctx *c, int d, const double *Y, double *Ki, double *ws, const HessJob &hj,
                      const double *y, double h, double s, const double **sums)
{
    if (d < 1 || d > BQ_MAXD || (hj.npad % 64))
        return fail(c, BQ_ERR_BAD_ARG, "logml_hess: d in [1, %d], npad a multiple of 64", BQ_MAXD);
    *sums = ws + hess_off_sums(hj.npad, d);
    switch (d) {
    case 1: return hess_run<1>(c, Y, Ki, ws, hj, y, h, s);
    case 2: return hess_run<2>(c, Y, Ki, ws, hj, y, h, s);
    case 3: return hess_run<3>(c, Y, Ki, ws, hj, y, h, s);
    case 4: return hess_run<4>(c, Y, Ki, ws, hj, y, h, s);
    case 5: return hess_run<5>(c, Y, Ki, ws, hj, y, h, s);
    case 6: return hess_run<6>(c, Y, Ki, ws, hj, y, h, s);
    case 7: return hess_run<7>(c, Y, Ki, ws, hj, y, h, s);
    default: return hess_run<8>(c, Y, Ki, ws, hj, y, h, s);
    }
}

} // namespace bqh
