// probe.hip -- hardware probes of libbqhip_probe.so (MFMA / FMA / HBM rates, launch latency,
// operand layouts, the diagonal factor's and a plan's timelines) and their kernels (probe.h).
// Not linked into libbqhip.so (Makefile).
#include "host.h"

#pragma GCC visibility push(default)
#include "../../include/bqhip_probe.h"
#pragma GCC visibility pop

#include "probe.h"

using namespace bqh;

// ===========================================================================
// hardware probes
// ===========================================================================
extern "C" int bq_probe_mfma_f64(bq_ctx *c, double *tflops)
{
    if (!c || !tflops)
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf o;
    HIPCHK(c, o.alloc(64));
    const int iters = 4096, blocks = c->cus * 8; // 2 waves per SIMD
    hipLaunchKernelGGL(probe_mfma_kernel, dim3(blocks), dim3(256), 0, c->stream, o.d(), 64);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    BQCHK(bq_timer_start(c));
    hipLaunchKernelGGL(probe_mfma_kernel, dim3(blocks), dim3(256), 0, c->stream, o.d(), iters);
    BQCHK(bq_timer_stop_ms(c, &ms));
    const double flops = (double)blocks * 4 /*waves*/ * iters * 4 /*mfma*/ * (16.0 * 16 * 4 * 2);
    *tflops = flops / (ms * 1e-3) / 1e12;
    return BQ_OK;
}

extern "C" int bq_probe_fma_f64(bq_ctx *c, double *tflops)
{
    if (!c || !tflops)
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf o;
    HIPCHK(c, o.alloc(64));
    const int iters = 1 << 16, blocks = c->cus * 8;
    hipLaunchKernelGGL(probe_fma_kernel, dim3(blocks), dim3(256), 0, c->stream, o.d(), 64);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    BQCHK(bq_timer_start(c));
    hipLaunchKernelGGL(probe_fma_kernel, dim3(blocks), dim3(256), 0, c->stream, o.d(), iters);
    BQCHK(bq_timer_stop_ms(c, &ms));
    const double flops = (double)blocks * 256 * (double)iters * 8 * 2;
    *tflops = flops / (ms * 1e-3) / 1e12;
    return BQ_OK;
}

extern "C" int bq_probe_hbm(bq_ctx *c, size_t bytes, double *write_gbs, double *copy_gbs)
{
    if (!c || bytes < 4096)
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf a, b;
    HIPCHK(c, a.alloc(bytes));
    HIPCHK(c, b.alloc(bytes));
    const size_t n2 = bytes / 16;
    const int blocks = c->cus * 8;
    float ms = 0;
    for (int rep = 0; rep < 2; ++rep) {
        BQCHK(bq_timer_start(c));
        for (int i = 0; i < 5; ++i)
            hipLaunchKernelGGL(probe_write_kernel, dim3(blocks), dim3(256), 0, c->stream,
                               static_cast<double2_t *>(a.p), n2);
        BQCHK(bq_timer_stop_ms(c, &ms));
    }
    if (write_gbs)
        *write_gbs = 5.0 * bytes / (ms * 1e-3) / 1e9;
    for (int rep = 0; rep < 2; ++rep) {
        BQCHK(bq_timer_start(c));
        for (int i = 0; i < 5; ++i)
            hipLaunchKernelGGL(probe_copy_kernel, dim3(blocks), dim3(256), 0, c->stream,
                               static_cast<double2_t *>(b.p), static_cast<const double2_t *>(a.p),
                               n2);
        BQCHK(bq_timer_stop_ms(c, &ms));
    }
    if (copy_gbs)
        *copy_gbs = 5.0 * 2.0 * bytes / (ms * 1e-3) / 1e9;
    return BQ_OK;
}

// `reps` launches of probe_read8_kernel over a `bytes`-sized buffer: a known byte count in the
// single-vector sweeps' access pattern (8 B per lane, 512 contiguous bytes per wave), for the
// calibration of rocprofv3's FETCH_SIZE on that pattern (tools/r06_profiles.sh, pass `calib`)
extern "C" int bq_probe_hbm_read8(bq_ctx *c, size_t bytes, int64_t reps, double *read_gbs)
{
    if (!c || bytes < 4096 || reps < 1)
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf a, o;
    HIPCHK(c, a.alloc(bytes));
    HIPCHK(c, o.alloc(64));
    HIPCHK(c, hipMemsetAsync(a.p, 0, bytes, c->stream));
    const size_t n = bytes / 8;
    float ms = 0;
    hipLaunchKernelGGL(probe_read8_kernel, dim3(c->cus * 2), dim3(1024), 0, c->stream, a.d(), n,
                       o.d());
    BQCHK(bq_timer_start(c));
    for (int64_t i = 0; i < reps; ++i)
        hipLaunchKernelGGL(probe_read8_kernel, dim3(c->cus * 2), dim3(1024), 0, c->stream, a.d(),
                           n, o.d());
    BQCHK(bq_timer_stop_ms(c, &ms));
    HIPCHK(c, hipGetLastError());
    if (read_gbs)
        *read_gbs = (double)reps * bytes / (ms * 1e-3) / 1e9;
    return BQ_OK;
}

// the probes' product on packed batch elements: C ldc x n, P ldp x k, Q ldq x k -- or, qt, Q given
// k-contiguous, ldq x n
static GemmJob probe_job(double *C, long ldc, const double *P, long ldp, const double *Q, long ldq,
                         int m, int n, int k, int lower, int batch, int qt)
{
    GemmJob g;
    g.C = C, g.ldc = ldc, g.cstride = ldc * n;
    g.P = P, g.ldp = ldp, g.pstride = ldp * k;
    g.Q = Q, g.qsj = qt ? ldq : 1, g.qsk = qt ? 1 : ldq, g.qstride = ldq * (qt ? n : k);
    g.m = m, g.n = n, g.k = k;
    g.lower = lower, g.batch = batch;
    return g;
}

// C (m x n) -= P (m x k) Q (n x k)^T on scratch operands through launch_gemm (the engine's own
// kernel selection): average ms over `reps` back-to-back launches.  qt: Q given k-contiguous.
extern "C" int bq_probe_gemm(bq_ctx *c, int64_t m, int64_t n, int64_t k, int lower, int64_t batch,
                             int qt, int64_t reps, double *ms_out)
{
    if (!c || !ms_out || m < 16 || n < 16 || k < 8 || batch < 1 || reps < 1)
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf C, P, Q;
    const long ldc = m, ldp = m, ldq = qt ? k : n;
    HIPCHK(c, C.alloc(sizeof(double) * (size_t)ldc * n * batch));
    HIPCHK(c, P.alloc(sizeof(double) * (size_t)ldp * k * batch));
    HIPCHK(c, Q.alloc(sizeof(double) * (size_t)n * k * batch));
    HIPCHK(c, hipMemsetAsync(C.p, 0, C.bytes, c->stream));
    hipLaunchKernelGGL(probe_fill_kernel, dim3(2048), dim3(256), 0, c->stream, P.d(),
                       P.bytes / sizeof(double), 1u);
    hipLaunchKernelGGL(probe_fill_kernel, dim3(2048), dim3(256), 0, c->stream, Q.d(),
                       Q.bytes / sizeof(double), 77u);
    HIPCHK(c, hipGetLastError());
    const GemmJob g = probe_job(C.d(), ldc, P.d(), ldp, Q.d(), ldq, (int)m, (int)n, (int)k, lower,
                                (int)batch, qt);
    BQCHK(launch_gemm(c, BQ_K_GEMM, g));
    float ms = 0;
    BQCHK(bq_timer_start(c));
    for (int64_t i = 0; i < reps; ++i)
        BQCHK(launch_gemm(c, BQ_K_GEMM, g));
    BQCHK(bq_timer_stop_ms(c, &ms));
    *ms_out = ms / (double)reps;
    return BQ_OK;
}

// ONE product on the caller's own operands, and the route it took (GemmRoute; bqhip_probe.h).
// Without operands nothing is launched: route[] is gemm_route's answer for the shape.
extern "C" int bq_probe_gemm_product(bq_ctx *c, double *C, int64_t ldc, const double *P, int64_t ldp,
                                     const double *Q, int64_t ldq, int64_t m, int64_t n, int64_t k,
                                     int lower, int64_t batch, int qt, int64_t ccut, int sharing,
                                     int want_fuse, int64_t j0, int seed_d, int rows, double *dinv,
                                     int32_t *info, int32_t *route)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!route)
        return fail(c, BQ_ERR_BAD_ARG, "gemm_product: null route");
    if (m < 16 || (m & 15) || n < 16 || (n & 15) || k < 8 || (k & 7) || m > 65536 || n > 65536 ||
        k > 65536 || batch < 1 || batch > 65535 || ccut < 0 || ccut > 65536)
        return fail(c, BQ_ERR_BAD_ARG, "gemm_product: m, n multiples of 16 and k of 8");
    if (sharing < 0 || sharing > 2 || seed_d < 0 || seed_d > 3)
        return fail(c, BQ_ERR_BAD_ARG, "gemm_product: sharing in 0 .. 2, seed_d in 0 .. 3");
    if (want_fuse && (m < 64 || n < 64 || j0 < 0 || j0 > (1 << 30)))
        return fail(c, BQ_ERR_BAD_ARG, "gemm_product: a fused factor needs a leading 64 x 64 block");
    if (rows && (lower || batch != 1 || seed_d || want_fuse))
        return fail(c, BQ_ERR_BAD_ARG, "gemm_product: a sweep's product is one full matrix");
    const bool run = C || P || Q;
    if (run && (!C || !P || !Q || ldc < m || ldp < m || ldq < (qt ? k : n) || seed_d > 0 ||
                (want_fuse && (!dinv || !info))))
        return fail(c, BQ_ERR_BAD_ARG,
                    "gemm_product: all three operands with their leading dimensions, no seed");
    HIPCHK(c, hipSetDevice(c->device));
    Sharing scope(c, sharing);
    GramSeed sd{};
    sd.d = seed_d;
    GemmRoute ran{};
    DevBuf Cd, Pd, Qd, dv, inf;
    if (run) {
        HIPCHK(c, Cd.alloc(sizeof(double) * (size_t)ldc * n * batch));
        HIPCHK(c, Pd.alloc(sizeof(double) * (size_t)ldp * k * batch));
        HIPCHK(c, Qd.alloc(sizeof(double) * (size_t)ldq * (qt ? n : k) * batch));
        HIPCHK(c, dv.alloc(sizeof(double) * BQ_DINV_STRIDE * (size_t)batch));
        HIPCHK(c, inf.alloc(sizeof(int) * (size_t)batch));
        HIPCHK(c, hipMemcpyAsync(Cd.p, C, Cd.bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(Pd.p, P, Pd.bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(Qd.p, Q, Qd.bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(dv.p, 0, dv.bytes, c->stream));
        HIPCHK(c, hipMemsetAsync(inf.p, 0, inf.bytes, c->stream));
    }
    GemmJob g = probe_job(Cd.d(), (long)ldc, Pd.d(), (long)ldp, Qd.d(), (long)ldq, (int)m, (int)n,
                          (int)k, lower, (int)batch, qt);
    g.ccut = (int)ccut;
    g.rows = rows != 0;
    if (seed_d)
        g.seed = &sd;
    if (want_fuse)
        g.fuse = {(int)j0, dv.d(), BQ_DINV_STRIDE, inf.i()};
    if (run)
        BQCHK(launch_gemm(c, BQ_K_GEMM, g, &ran));
    else
        ran = gemm_route(c, g);
    const int32_t r[8] = {(int32_t)ran.kernel, ran.mfma, ran.fused, ran.seeded, ran.assemble_first,
                          (int32_t)ran.grid.x, (int32_t)ran.grid.y, (int32_t)ran.grid.z};
    std::memcpy(route, r, sizeof r);
    if (!run)
        return BQ_OK;
    HIPCHK(c, hipMemcpyAsync(C, Cd.p, Cd.bytes, hipMemcpyDeviceToHost, c->stream));
    if (ran.fused) {
        // (the reciprocal pivots: the first 64 doubles of every record)
        HIPCHK(c, hipMemcpy2DAsync(dinv, sizeof(double) * 64, dv.p, sizeof(double) * BQ_DINV_STRIDE,
                                   sizeof(double) * 64, batch, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(info, inf.p, inf.bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// kind 0: v_mfma_f64_16x16x4_f64, 1: v_mfma_f64_4x4x4_4b_f64; nacc in {1,2,4,8};
// blocks_per_cu 256-thread blocks per CU (= waves per SIMD)
extern "C" int bq_probe_mfma_variant(bq_ctx *c, int kind, int nacc, int blocks_per_cu,
                                     double *tflops)
{
    if (!c || !tflops || blocks_per_cu < 1 || blocks_per_cu > 8)
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf o;
    HIPCHK(c, o.alloc(64));
    if (kind == 4 || kind == 5) {
        // the GEMM inner step SUSTAINED: 300 launches of ~1 ms back to back, the last 200 timed;
        // kind 4: operands near 1.0 (few mantissa bits set), kind 5: random mantissas
        const int it = 1024, blocks = c->cus * blocks_per_cu;
        float ms = 0;
        for (int rep = 0; rep < 300; ++rep) {
            if (rep == 100)
                BQCHK(bq_timer_start(c));
            if (kind == 4)
                hipLaunchKernelGGL((probe_mfma_step_kernel<0, 0>), dim3(blocks), dim3(256), 0,
                                   c->stream, o.d(), it);
            else
                hipLaunchKernelGGL((probe_mfma_step_kernel<0, 1>), dim3(blocks), dim3(256), 0,
                                   c->stream, o.d(), it);
        }
        BQCHK(bq_timer_stop_ms(c, &ms));
        *tflops = 200.0 * (double)blocks * 4 * (double)it * 64 * 512.0 / (ms * 1e-3) / 1e12;
        return BQ_OK;
    }
    if (kind >= 2) { // the GEMM inner step, kind 2: no rotations, 3: with rotations
        const int it = 512, blocks = c->cus * blocks_per_cu;
        float ms = 0;
        for (int rep = 0; rep < 2; ++rep) {
            BQCHK(bq_timer_start(c));
            if (kind == 2)
                hipLaunchKernelGGL((probe_mfma_step_kernel<0, 0>), dim3(blocks), dim3(256), 0,
                                   c->stream, o.d(), it);
            else
                hipLaunchKernelGGL((probe_mfma_step_kernel<1, 0>), dim3(blocks), dim3(256), 0,
                                   c->stream, o.d(), it);
            BQCHK(bq_timer_stop_ms(c, &ms));
        }
        *tflops = (double)blocks * 4 * (double)it * 64 * 512.0 / (ms * 1e-3) / 1e12;
        return BQ_OK;
    }
    const int iters = 8192 / nacc, blocks = c->cus * blocks_per_cu;
    auto launch = [&](int it) {
#define PV(K_, N_)                                                                                 \
    hipLaunchKernelGGL((probe_mfma_var_kernel<K_, N_>), dim3(blocks), dim3(256), 0, c->stream,     \
                       o.d(), it)
        if (kind == 0) {
            switch (nacc) {
            case 1: PV(0, 1); break;
            case 2: PV(0, 2); break;
            case 4: PV(0, 4); break;
            default: PV(0, 8); break;
            }
        } else {
            switch (nacc) {
            case 1: PV(1, 1); break;
            case 2: PV(1, 2); break;
            case 4: PV(1, 4); break;
            default: PV(1, 8); break;
            }
        }
#undef PV
    };
    launch(16);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    BQCHK(bq_timer_start(c));
    launch(iters);
    BQCHK(bq_timer_stop_ms(c, &ms));
    const double per = kind == 0 ? 16.0 * 16 * 4 * 2 : 4.0 * 4 * 4 * 4 * 2;
    const int na = (nacc == 1 || nacc == 2 || nacc == 4) ? nacc : 8;
    *tflops = (double)blocks * 4 * (double)iters * na * per / (ms * 1e-3) / 1e12;
    return BQ_OK;
}

extern "C" int bq_probe_mfma444_layout(bq_ctx *c, int cbsz, int abid, int32_t *out8192)
{
    if (!c || !out8192)
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf o;
    HIPCHK(c, o.alloc(8192 * sizeof(int)));
#define PL(C_, A_)                                                                                 \
    hipLaunchKernelGGL((probe_layout444_kernel<C_, A_>), dim3(64, 64), dim3(64), 0, c->stream, o.i())
    if (cbsz == 0) PL(0, 0);
    else if (cbsz == 1 && abid == 0) PL(1, 0);
    else if (cbsz == 1) PL(1, 1);
    else if (abid == 0) PL(2, 0);
    else if (abid == 1) PL(2, 1);
    else if (abid == 2) PL(2, 2);
    else PL(2, 3);
#undef PL
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out8192, o.p, 8192 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

extern "C" int bq_probe_exp(bq_ctx *c, const double *x, int64_t n, double *out)
{
    if (!c || !x || !out || n < 1 || n > (1 << 28))
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf xd, od;
    HIPCHK(c, xd.alloc(sizeof(double) * n));
    HIPCHK(c, od.alloc(sizeof(double) * n));
    HIPCHK(c, hipMemcpyAsync(xd.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(probe_exp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       xd.d(), od.d(), (int)n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, od.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// The diagonal factor alone: A (64 x 64 host, column-major) is factored `reps` times from a
// resident copy; L_out / dinv_out (BQ_DINV_HALF doubles) / info_out are the last launch's
// results, us_per_launch the HIP-event average, stamps5 the in-kernel s_memtime stamps
// (entry, block loaded, pivot chain done, sub-blocks in LDS, end; shader cycles) followed at
// [8 + 2 (4 P + w) + k] by wave w's arrival at (k = 0) / release from (k = 1) the barrier that
// publishes panel P: 136 values.
extern "C" int bq_probe_potf2(bq_ctx *c, const double *A, int from_lds, int64_t reps,
                              double *L_out, double *dinv_out, int32_t *info_out,
                              double *us_per_launch, int64_t *stamps5)
{
    if (!c || !A || reps < 1)
        return BQ_ERR_BAD_ARG;
    // from_lds bits 8-14: the block's real columns when fewer than 64 (the padded epilogue)
    const int nreal = ((from_lds >> 8) & 127) ? ((from_lds >> 8) & 127) : 64;
    if (nreal > 64)
        return fail(c, BQ_ERR_BAD_ARG, "potf2: at most 64 real columns");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf ain, a, dv, inf, st;
    HIPCHK(c, ain.alloc(sizeof(double) * 4096));
    HIPCHK(c, a.alloc(sizeof(double) * 4096));
    HIPCHK(c, dv.alloc(sizeof(double) * BQ_DINV_STRIDE));
    HIPCHK(c, inf.alloc(64));
    HIPCHK(c, st.alloc(sizeof(long long) * 136));
    HIPCHK(c, hipMemcpyAsync(ain.p, A, sizeof(double) * 4096, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(inf.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(a.p, 0, sizeof(double) * 4096, c->stream));
    // from_lds bit 2: per-wave barrier stamps as well (four-wave form; stamps[5] is the switch)
    {
        const long long flag = (from_lds & 4) ? 1 : 0;
        HIPCHK(c, hipMemsetAsync(st.p, 0, sizeof(long long) * 136, c->stream));
        HIPCHK(c, hipMemcpyAsync(static_cast<long long *>(st.p) + 5, &flag, sizeof flag,
                                 hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    auto launch = [&]() {
        // from_lds bit 1: the eight-wave form
        if (from_lds & 2)
            hipLaunchKernelGGL(potf2_probe_kernel<8>, dim3(1), dim3(512), 0, c->stream, ain.d(),
                               a.d(), 64L, dv.d(), inf.i(), static_cast<long long *>(st.p),
                               from_lds & 1, nreal);
        else
            hipLaunchKernelGGL(potf2_probe_kernel<4>, dim3(1), dim3(256), 0, c->stream, ain.d(),
                               a.d(), 64L, dv.d(), inf.i(), static_cast<long long *>(st.p),
                               from_lds & 1, nreal);
    };
    for (int i = 0; i < 5; ++i)
        launch();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemsetAsync(inf.p, 0, 64, c->stream));
    float ms = 0;
    BQCHK(bq_timer_start(c));
    for (int64_t i = 0; i < reps; ++i)
        launch();
    BQCHK(bq_timer_stop_ms(c, &ms));
    HIPCHK(c, hipGetLastError());
    if (us_per_launch)
        *us_per_launch = ms * 1e3 / (double)reps;
    if (L_out)
        HIPCHK(c, hipMemcpyAsync(L_out, a.p, sizeof(double) * 4096, hipMemcpyDeviceToHost,
                                 c->stream));
    if (dinv_out)
        HIPCHK(c, hipMemcpyAsync(dinv_out, dv.p, sizeof(double) * BQ_DINV_HALF,
                                 hipMemcpyDeviceToHost, c->stream));
    if (info_out)
        HIPCHK(c, hipMemcpyAsync(info_out, inf.p, sizeof(int32_t), hipMemcpyDeviceToHost,
                                 c->stream));
    if (stamps5)
        HIPCHK(c, hipMemcpyAsync(stamps5, st.p, sizeof(int64_t) * 136, hipMemcpyDeviceToHost,
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

extern "C" int bq_probe_launch(bq_ctx *c, int64_t n, double *us_per_launch)
{
    if (!c || !us_per_launch || n < 1)
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf o;
    HIPCHK(c, o.alloc(64));
    for (int i = 0; i < 10; ++i)
        hipLaunchKernelGGL(probe_empty_kernel, dim3(1), dim3(64), 0, c->stream, o.d());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    BQCHK(bq_timer_start(c));
    for (int64_t i = 0; i < n; ++i)
        hipLaunchKernelGGL(probe_empty_kernel, dim3(1), dim3(64), 0, c->stream, o.d());
    BQCHK(bq_timer_stop_ms(c, &ms));
    *us_per_launch = ms * 1e3 / (double)n;
    return BQ_OK;
}

// ns per hand-off (one direction) of probe_hop_kernel's eight ping-pong pairs, the pairs' XCC ids
// and the payload words that arrived wrong; BQ_ERR_HIP if a partner never answered
extern "C" int bq_probe_xcd_hop(bq_ctx *c, int mode, int64_t iters, int64_t kib, double *ns_per_hop,
                                int32_t *xcc16, int64_t *bad_words)
{
    if (!c || !ns_per_hop || !xcc16 || !bad_words || mode < 0 || mode > 2 || iters < 1 ||
        iters > 100000 || kib < 1 || kib > 64)
        return c ? fail(c, BQ_ERR_BAD_ARG, "xcd_hop: mode 0..2, 1..100000 iterations, 1..64 KiB")
                 : BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf flags, pay, out, xcc, bad, err;
    HIPCHK(c, flags.alloc(sizeof(unsigned) * 64 * 16));
    HIPCHK(c, pay.alloc(sizeof(double) * 128 * (size_t)kib * 16));
    HIPCHK(c, out.alloc(sizeof(long long) * 16));
    HIPCHK(c, xcc.alloc(sizeof(int) * 16));
    HIPCHK(c, bad.alloc(sizeof(int) * 16));
    HIPCHK(c, err.alloc(sizeof(int)));
    HIPCHK(c, hipMemsetAsync(flags.p, 0, flags.bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(pay.p, 0, pay.bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(err.p, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(probe_hop_kernel, dim3(16), dim3(64), 0, c->stream,
                       static_cast<unsigned *>(flags.p), pay.d(), (int)iters, mode, (int)kib,
                       static_cast<long long *>(out.p), xcc.i(), bad.i(), err.i());
    HIPCHK(c, hipGetLastError());
    long long ho[16];
    int hb[16], he = 0;
    HIPCHK(c, hipMemcpyAsync(ho, out.p, sizeof ho, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(xcc16, xcc.p, sizeof(int) * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hb, bad.p, sizeof hb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&he, err.p, sizeof he, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (he)
        return fail(c, BQ_ERR_HIP, "xcd_hop: a partner never answered (bounded spin ran out)");
    long long worst = 0;
    *bad_words = 0;
    for (int b = 0; b < 16; ++b) {
        worst = std::max(worst, ho[b]);
        *bad_words += hb[b];
    }
    *ns_per_hop = (double)worst * 10.0 / (2.0 * (double)iters); // 100 MHz ticks
    return BQ_OK;
}

extern "C" int bq_probe_mfma_layout(bq_ctx *c, double *out256)
{
    if (!c || !out256)
        return BQ_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf o;
    HIPCHK(c, o.alloc(256 * sizeof(double)));
    hipLaunchKernelGGL(probe_layout_kernel, dim3(1), dim3(64), 0, c->stream, o.d());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out256, o.p, 256 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// The batched panel solve alone: X (m x kb per problem) <- X L^-T against `batch` lower-triangular
// kb x kb factors L (host, column-major, dense lower triangles), through the launches the batched
// factorisation issues for an outer block (mode 0: as the context is configured; 1: the recursive
// products + solves; 2: the one-launch sweep).  The factors' block-inverse records are built on
// the device (diag_winv_kernel).
extern "C" int bq_probe_panel_solve(bq_ctx *c, int64_t m, int64_t kb, int64_t batch, const double *L,
                                    double *X, int mode, int64_t reps, double *ms_per_call)
{
    if (!c || !L || !X || m < 64 || (m & 63) || kb < 64 || (kb & 63) || batch < 1)
        return c ? fail(c, BQ_ERR_BAD_ARG, "panel_solve: m, kb multiples of 64") : BQ_ERR_BAD_ARG;
    if (mode < 0 || mode > 2)
        return fail(c, BQ_ERR_BAD_ARG, "panel_solve: mode must be 0, 1 or 2");
    HIPCHK(c, hipSetDevice(c->device));
    const long lda = (long)(kb + m), astride = lda * (long)kb;
    const long rstride = (long)(kb / 64) * BQ_DINV_HALF;
    DevBuf A, rec;
    HIPCHK(c, A.alloc(sizeof(double) * (size_t)astride * batch));
    HIPCHK(c, rec.alloc(sizeof(double) * (size_t)rstride * batch));
    for (int64_t b = 0; b < batch; ++b) {
        HIPCHK(c, hipMemcpy2DAsync(A.d() + b * astride, sizeof(double) * lda, L + b * kb * kb,
                                   sizeof(double) * kb, sizeof(double) * kb, kb,
                                   hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(A.d() + b * astride + kb, sizeof(double) * lda, X + b * m * kb,
                                   sizeof(double) * m, sizeof(double) * m, kb,
                                   hipMemcpyHostToDevice, c->stream));
        BQCHK(launch_diag_winv(c, A.d() + b * astride, lda, (int)kb, rec.d() + b * rstride));
    }
    const bool one_launch = mode == 0 ? c->cfg.df_sweep != 0 : mode == 2;
    const int st = enqueue_panel_solve(c, A.d(), lda, astride, (int)batch, (int)kb, (int)m, 0,
                                       (int)kb, rec.d(), rstride, one_launch);
    if (st == BQ_OK && reps > 0 && ms_per_call) {
        // timing: the same call again and again on its own (now solved, still finite) output
        float ms = 0;
        BQCHK(bq_timer_start(c));
        for (int64_t r = 0; r < reps; ++r)
            (void)enqueue_panel_solve(c, A.d(), lda, astride, (int)batch, (int)kb, (int)m, 0,
                                      (int)kb, rec.d(), rstride, one_launch);
        BQCHK(bq_timer_stop_ms(c, &ms));
        *ms_per_call = ms / (double)reps;
        return BQ_OK; // (X is not downloaded: it has been solved reps + 1 times)
    }
    BQCHK(st);
    for (int64_t b = 0; b < batch; ++b)
        HIPCHK(c, hipMemcpy2DAsync(X + b * m * kb, sizeof(double) * m, A.d() + b * astride + kb,
                                   sizeof(double) * lda, sizeof(double) * m, kb,
                                   hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// The batched sweep on the caller's own matrices (a plan takes points, not matrices): the first
// ncols columns of `batch` lower ntot x ntot matrices are eliminated along the route sweep_route
// picks for them, with the workspace sized as plan_create sizes it and default SweepArgs (nothing
// seeded, no folded read-out, the border x border Schur complement computed).  The whole buffer --
// padding rows and the gaps between matrices included -- goes up and comes back verbatim.
extern "C" int bq_probe_potrf_batch(bq_ctx *c, int64_t batch, int64_t ntot, int64_t ncols,
                                    int64_t lda, int64_t astride, double *A, int32_t *info,
                                    int32_t *route)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!A || !info || !route || batch < 1 || batch > (1 << 20) || ntot < 64 || ntot > 65536 ||
        (ntot & 63) || ncols < 64 || (ncols & 63) || ncols > ntot)
        return fail(c, BQ_ERR_BAD_ARG, "potrf_batch: ntot, ncols multiples of 64, ncols <= ntot");
    if (lda == 0)
        lda = pick_ld(ntot);
    if (astride == 0)
        astride = lda * ntot;
    if (lda < ntot || (lda & 1) || astride < lda * ntot || (astride & 1))
        return fail(c, BQ_ERR_BAD_ARG, "potrf_batch: lda >= ntot, astride >= lda ntot, both even");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf Ad, dinv, ws, inf;
    const size_t abytes = sizeof(double) * (size_t)astride * (size_t)batch;
    HIPCHK(c, Ad.alloc(abytes));
    HIPCHK(c, dinv.alloc(sizeof(double) * BQ_DINV_STRIDE * (size_t)batch));
    HIPCHK(c, ws.alloc(sizeof(double) *
                       sweep_route(c, (int)ntot, (int)ntot, (int)batch).ws_doubles));
    HIPCHK(c, inf.alloc(sizeof(int) * (size_t)batch));
    const SweepRoute r =
        sweep_route(c, (int)ntot, (int)ncols, (int)batch, ws.bytes / sizeof(double));
    route[0] = (int32_t)r.kind;
    route[1] = r.nb;
    route[2] = r.ws_doubles != 0;
    HIPCHK(c, hipMemcpyAsync(Ad.p, A, abytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(inf.p, 0, sizeof(int) * (size_t)batch, c->stream));
    BQCHK(enqueue_potrf_partial(c, r, Ad.d(), (long)lda, (long)astride, dinv.d(), inf.i(), ws.d()));
    HIPCHK(c, hipMemcpyAsync(A, Ad.p, abytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(info, inf.p, sizeof(int32_t) * (size_t)batch, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// Both producers of a factor's block-inverse records on one matrix: A (128 x 128 host, column-major,
// ld 128, SPD) is factored by the one-launch steps, whose two records stay behind in the two halves
// of the sweep's ping-pong, and the resident factor's records are then built from the factor in
// memory (diag_winv_kernel) as a fit builds them.
extern "C" int bq_probe_records(bq_ctx *c, double *A, double *rec_sweep, double *rec_resident,
                                int32_t *info)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!A || !rec_sweep || !rec_resident || !info)
        return fail(c, BQ_ERR_BAD_ARG, "records: null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    const int ntot = 128;
    const long lda = ntot, astride = lda * ntot;
    DevBuf Ad, dinv, dw, ws, inf;
    HIPCHK(c, Ad.alloc(sizeof(double) * (size_t)astride));
    HIPCHK(c, dinv.alloc(sizeof(double) * BQ_DINV_STRIDE));
    HIPCHK(c, dw.alloc(sizeof(double) * BQ_DINV_STRIDE));
    HIPCHK(c, ws.alloc(sizeof(double) * sweep_route(c, ntot, ntot, 1).ws_doubles));
    HIPCHK(c, inf.alloc(sizeof(int)));
    const SweepRoute r = sweep_route(c, ntot, ntot, 1, ws.bytes / sizeof(double));
    if (r.kind != SweepRoute::Slab)
        return fail(c, BQ_ERR_BAD_ARG, "records: the context does not run the one-launch steps");
    HIPCHK(c, hipMemcpyAsync(Ad.p, A, sizeof(double) * (size_t)astride, hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipMemsetAsync(inf.p, 0, sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(dinv.p, 0xA5, dinv.bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(dw.p, 0xA5, dw.bytes, c->stream));
    BQCHK(enqueue_potrf_partial(c, r, Ad.d(), lda, astride, dinv.d(), inf.i(), ws.d()));
    BQCHK(launch_diag_winv(c, Ad.d(), lda, ntot, dw.d()));
    HIPCHK(c, hipMemcpyAsync(A, Ad.p, sizeof(double) * (size_t)astride, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(rec_sweep, dinv.p, dinv.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(rec_resident, dw.p, dw.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(info, inf.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// ONE sweep over a resident factor on the caller's own factor and right-hand sides (a fit takes
// points, bq_cho_solve always runs both sweeps): L (n x n host, column-major, lower) goes up with
// leading dimension ldl, the 16 x 16 and the wide inverses are built as bq_cho_solve builds them,
// the sweep `which` runs on X (right-hand sides as ROWS, X[r + j ldx]) and the whole ldx x n buffer
// comes back.  route: what the sweep reported it ran (RowsRoute), not a second opinion.
extern "C" int bq_probe_sweep(bq_ctx *c, int which, int64_t n, const double *L, int64_t ldl,
                              int64_t mrows, int64_t ldx, double *X, int32_t *route)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!L || !X || !route)
        return fail(c, BQ_ERR_BAD_ARG, "sweep: null pointer");
    if (which < BQ_SWEEP_FORWARD_ROWS || which > BQ_SWEEP_BACKWARD_VEC_FLOW)
        return fail(c, BQ_ERR_BAD_ARG, "sweep: which must be 0 .. %d", BQ_SWEEP_BACKWARD_VEC_FLOW);
    if (n < 64 || n > 65536 || (n & 63))
        return fail(c, BQ_ERR_BAD_ARG, "sweep: n must be a multiple of 64 in [64, 65536]");
    if (ldl == 0)
        ldl = pick_ld(n);
    if (ldl < n)
        return fail(c, BQ_ERR_BAD_ARG, "sweep: ldl >= n (0: the engine's own)");
    const bool vec = which >= BQ_SWEEP_FORWARD_VEC, flow = which >= BQ_SWEEP_FORWARD_VEC_FLOW;
    const bool inverse = which == BQ_SWEEP_INVERSE_ROWS;
    if (vec ? mrows != 1 : (mrows < 32 || (mrows & 31) || mrows > 65536))
        return fail(c, BQ_ERR_BAD_ARG, "sweep: mrows a multiple of 32 (single-vector sweeps: 1)");
    if (ldx < mrows || ldx > 65536)
        return fail(c, BQ_ERR_BAD_ARG, "sweep: ldx >= mrows");
    if (inverse && (mrows != n || ldx != n))
        return fail(c, BQ_ERR_BAD_ARG, "sweep: the triangular inverse has mrows = ldx = n");
    const int npad = (int)n, B = wide_block(npad);
    if (flow && !trsv_flow_ok(c, npad, B))
        return fail(c, BQ_ERR_BAD_ARG, "sweep: no one-launch single-vector sweep at n = %d", npad);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf A, dw, wide;
    HIPCHK(c, A.alloc(sizeof(double) * (size_t)ldl * npad));
    HIPCHK(c, dw.alloc(sizeof(double) * BQ_DINV_HALF * (size_t)(npad / 64)));
    HIPCHK(c, wide.alloc(sizeof(double) * wide_alloc_doubles(npad)));
    HIPCHK(c, hipMemsetAsync(A.p, 0, A.bytes, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(A.p, sizeof(double) * ldl, L, sizeof(double) * n, sizeof(double) * n,
                               n, hipMemcpyHostToDevice, c->stream));
    BQCHK(launch_diag_winv(c, A.d(), ldl, npad, dw.d()));
    BQCHK(compute_wide_inverses(c, A.d(), ldl, npad, dw.d(), wide.d()));
    const WideInv w = wide_views(wide.d(), npad);
    RowsRoute ran{RowsRoute::Gemm, B, 0, 0};
    int kind = -1;
    if (vec) {
        // the vector is row 0 of X: X[j ldx]
        std::vector<double> h((size_t)npad);
        for (int j = 0; j < npad; ++j)
            h[(size_t)j] = X[(size_t)j * ldx];
        DevBuf Xd;
        HIPCHK(c, Xd.alloc(sizeof(double) *
                           (2 * (size_t)npad + (flow ? trsv_flow_ws_doubles(npad, B) : 0))));
        double *x = Xd.d(), *y = Xd.d() + npad, *fw = flow ? Xd.d() + 2 * (size_t)npad : nullptr;
        const bool forward = which == BQ_SWEEP_FORWARD_VEC || which == BQ_SWEEP_FORWARD_VEC_FLOW;
        // (as bq_cho_solve: a timed-out hand-off re-issues the sweep on the per-block kernels)
        BQCHK(with_flow_fallback(c, [&]() -> int {
            HIPCHK(c, hipMemsetAsync(Xd.p, 0, sizeof(double) * 2 * (size_t)npad, c->stream));
            HIPCHK(c, hipMemcpyAsync(x, h.data(), sizeof(double) * npad, hipMemcpyHostToDevice,
                                     c->stream));
            if (forward)
                BQCHK(enqueue_forward_vec(c, x, y, A.d(), ldl, npad, w, fw));
            else
                BQCHK(enqueue_backward_vec(c, x, y, A.d(), ldl, npad, w, fw));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return BQ_OK;
        }));
        HIPCHK(c, hipMemcpy(h.data(), y, sizeof(double) * npad, hipMemcpyDeviceToHost));
        for (int j = 0; j < npad; ++j)
            X[(size_t)j * ldx] = h[(size_t)j];
        kind = flow ? BQ_SWEEP_KIND_VEC_FLOW : BQ_SWEEP_KIND_VEC_BLOCK;
    } else {
        // both buffers start as the caller's: whichever holds the result, its rows mrows .. ldx - 1
        // are the caller's bits unless a kernel wrote them
        DevBuf X1, X2;
        const size_t xbytes = sizeof(double) * (size_t)ldx * npad;
        HIPCHK(c, X1.alloc(xbytes));
        HIPCHK(c, X2.alloc(xbytes));
        double *res = X2.d();
        if (inverse) {
            // (Y's strict lower triangle is not written: cleared as fit_y clears it)
            HIPCHK(c, hipMemsetAsync(X2.p, 0, xbytes, c->stream));
            BQCHK(enqueue_inverse_rows(c, X1.d(), X2.d(), A.d(), ldl, npad, w, &ran));
            kind = (int)ran.kind;
        } else {
            HIPCHK(c, hipMemcpyAsync(X1.p, X, xbytes, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(X2.p, X, xbytes, hipMemcpyHostToDevice, c->stream));
            if (which == BQ_SWEEP_FORWARD_ROWS) {
                BQCHK(enqueue_forward_rows(c, X1.d(), X2.d(), ldx, (int)mrows, A.d(), ldl, npad, w,
                                           &ran));
                kind = (int)ran.kind;
            } else if (which == BQ_SWEEP_BACKWARD_ROWS) {
                BQCHK(enqueue_backward_rows(c, X1.d(), X2.d(), ldx, (int)mrows, A.d(), ldl, npad, w,
                                            &ran));
                kind = (int)ran.kind;
            } else {
                BQCHK(enqueue_forward_rows_blk(c, X1.d(), ldx, (int)mrows, A.d(), ldl, npad,
                                               dw.d()));
                res = X1.d();
                ran.B = 64;
                kind = BQ_SWEEP_KIND_BLK;
            }
        }
        HIPCHK(c, hipMemcpyAsync(X, res, xbytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    route[0] = kind;
    route[1] = ran.B;
    route[2] = ran.n_lds;
    route[3] = ran.n_splitk;
    route[4] = (int32_t)c->n_flow_fallback;
    return BQ_OK;
}

// The first launch of a small system's sweep alone (launch_assemble with a FirstStep), on the
// caller's points, targets and parameters, and everything it leaves in memory: the first block
// column of A (ntot rows x 64 columns per problem, the leading block's upper triangle included),
// the scratch column S0, the factor's record, the failure flags and scal.  Every buffer starts as
// 0xA5 bytes, so what the launch does not write comes back as that.  ntot, dinv_len: what the
// caller sized Acol / S0 and dinv for (checked).  stamps16 (d = 1 only; or
// null): the stamped instantiation's s_memtime values of workgroup (0, 0) of problem 0 --
// [0] entry, [1] leading block assembled, [2 .. 6] the factor's five (block held, first panel,
// chain done, epilogue entered, end).
extern "C" int bq_probe_first_launch(bq_ctx *c, int64_t batch, int64_t d, int64_t n, int64_t M,
                                     const double *x, const double *y, const double *xo, double h,
                                     const double *w, double s, int64_t ntot, int64_t dinv_len,
                                     double *Acol, double *S0, double *dinv, int32_t *info,
                                     double *scal, int64_t *stamps16)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    BQCHK(check_dims(c, d, n));
    if (batch < 1 || batch > 65535 || M < 0 || M > 4096 || !x || !y || (!xo && M) || !w || !Acol ||
        !S0 || !dinv || !info || !scal)
        return fail(c, BQ_ERR_BAD_ARG, "first_launch: illegal value");
    BQCHK(check_w(c, d, h, w, s));
    const Layout L = make_layout((int)n, (int)M, true);
    const long lda = pick_ld(L.ntot), astride = lda * (long)L.ntot;
    // (the caller sized Acol, S0 and dinv: it says for what)
    if (ntot != L.ntot || dinv_len != BQ_DINV_STRIDE)
        return fail(c, BQ_ERR_BAD_ARG, "first_launch: buffers for ntot = %d and %d doubles of record, not %lld and %lld",
                    L.ntot, (int)BQ_DINV_STRIDE, (long long)ntot, (long long)dinv_len);
    if (!sweep_route(c, L.ntot, L.npad, (int)batch, ~(size_t)0 >> 1).first_in_assembly)
        return fail(c, BQ_ERR_BAD_ARG, "first_launch: this shape's sweep has no first launch in the assembly");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf A, pts, yd, gp, dv, ws, inf, sc, st;
    HIPCHK(c, A.alloc(sizeof(double) * (size_t)astride * batch));
    HIPCHK(c, pts.alloc(sizeof(double) * (size_t)d * L.ntot * batch));
    HIPCHK(c, yd.alloc(sizeof(double) * (size_t)L.npad * batch));
    HIPCHK(c, gp.alloc(sizeof(GaussParams) * (size_t)batch));
    HIPCHK(c, dv.alloc(sizeof(double) * BQ_DINV_STRIDE * (size_t)batch));
    HIPCHK(c, ws.alloc(sizeof(double) * 64 * (size_t)L.ntot * batch));
    HIPCHK(c, inf.alloc(sizeof(int) * (size_t)batch));
    HIPCHK(c, sc.alloc(sizeof(double) * 4 * (size_t)batch));
    HIPCHK(c, st.alloc(sizeof(long long) * 16));
    for (DevBuf *b : {&A, &dv, &ws, &inf, &sc})
        HIPCHK(c, hipMemsetAsync(b->p, 0xA5, b->bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(pts.p, 0, pts.bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(yd.p, 0, yd.bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(st.p, 0, st.bytes, c->stream));
    std::vector<GaussParams> hgp((size_t)batch, make_params((int)d, h, w, s));
    HIPCHK(c, hipMemcpyAsync(gp.p, hgp.data(), gp.bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(pts.p, sizeof(double) * d * L.ntot, x, sizeof(double) * d * n,
                               sizeof(double) * d * n, batch, hipMemcpyHostToDevice, c->stream));
    if (M > 0)
        HIPCHK(c, hipMemcpy2DAsync(pts.d() + (size_t)d * L.npad, sizeof(double) * d * L.ntot, xo,
                                   sizeof(double) * d * M, sizeof(double) * d * M, batch,
                                   hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(yd.p, sizeof(double) * L.npad, y, sizeof(double) * n,
                               sizeof(double) * n, batch, hipMemcpyHostToDevice, c->stream));
    FirstStep fs;
    fs.S0 = ws.d();
    fs.lds = L.ntot;
    fs.sstride = 64L * L.ntot;
    fs.dinv = dv.d();
    fs.info = inf.i();
    fs.scal = sc.d();
    fs.stamps = stamps16 ? static_cast<long long *>(st.p) : nullptr;
    BQCHK(launch_assemble(c, (int)d, pts.d(), (long)d * L.ntot, yd.d(), L.npad,
                          static_cast<const GaussParams *>(gp.p), 1, A.d(), lda, astride, L,
                          (int)batch, fs));
    for (int64_t b = 0; b < batch; ++b)
        HIPCHK(c, hipMemcpy2DAsync(Acol + (size_t)b * 64 * L.ntot, sizeof(double) * L.ntot,
                                   A.d() + (size_t)b * astride, sizeof(double) * lda,
                                   sizeof(double) * L.ntot, 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(S0, ws.p, ws.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dinv, dv.p, dv.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(info, inf.p, inf.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(scal, sc.p, sc.bytes, hipMemcpyDeviceToHost, c->stream));
    if (stamps16)
        HIPCHK(c, hipMemcpyAsync(stamps16, st.p, st.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// One eager (not graph-replayed) pass of a plan with the profiling instantiation of the slab
// step: stamps[160 * step + k] = s_memtime of workgroup 0 at (0) entry, (1) factor fragments
// loaded, (2) panel rows solved, (3) tile loaded + Q in LDS, (4) tile updated, (5..9) the
// diagonal factor's entry / block in registers / pivot chain done / sub-blocks in LDS / end.
// The pipelined diagonal tile (BQ_DIAG_PIPE, slab.h): (2) wave 0 behind the barrier that
// publishes the last column block, (3) stays 0, (4) wave 4 behind its last MFMA, (16..18) /
// (19..21) wave 4's / wave 0's arrivals at the barriers of column blocks 1 .. 3.  (24..31) the
// stores, on s_memrealtime: workgroup 0's entry and end, one off-diagonal workgroup's entry,
// update and last store acknowledged (slab.h, BQ_SSTAMP_STORES; tools/c2_timeline.py).
extern "C" int bq_probe_c2_timeline(bq_ctx *c, bq_plan *p, int64_t *stamps, int64_t nsteps)
{
    if (!c || !p || !stamps || nsteps < 1 || nsteps > 1024)
        return BQ_ERR_BAD_ARG;
    // only the one-launch slab sweep carries the stamped instantiation, and it stamps one
    // record per step into the caller's nsteps (the sweep itself skips steps beyond them)
    if (sweep_route(c, p->L.ntot, p->L.npad, p->nprob, p->panel.bytes / sizeof(double)).kind !=
        SweepRoute::Slab)
        return fail(c, BQ_ERR_BAD_ARG, "timeline: this plan does not sweep with the one-launch steps");
    if (nsteps < p->L.npad / 64)
        return fail(c, BQ_ERR_BAD_ARG, "timeline: %d steps, room for %d", p->L.npad / 64, (int)nsteps);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf st;
    HIPCHK(c, st.alloc(sizeof(long long) * 160 * (size_t)nsteps));
    HIPCHK(c, hipMemsetAsync(st.p, 0, st.bytes, c->stream));
    BQCHK(plan_enqueue(c, p, static_cast<long long *>(st.p), (int)nsteps));
    HIPCHK(c, hipMemcpyAsync(stamps, st.p, st.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}
