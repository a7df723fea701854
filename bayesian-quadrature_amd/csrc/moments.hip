// moments.hip -- host side of the closed-form Gaussian-kernel integrals, of the BQ moments and
// of the acquisition entry points, with their kernels (moments.h).
//
// Reference: gauss_c.pyx:95-164,235-339,416-531,617-713 and bq_c.pyx:157-213,264-355.
// The d x d (or 2d x 2d) covariance algebra is done here on the host in plain
// loops; the per-point / per-pair work runs in the kernels of moments.h.
#include "host.h"
#include "moments.h"
#include "marginal.h"

using namespace bqh;

namespace {

constexpr int MAXF = 2 * BQ_MAXD;
constexpr double LOG_2PI = 1.8378770664093453;

// row-major small dense helpers, n <= MAXF
struct Small {
    int n = 0;
    double a[MAXF * MAXF] = {0};
    double &operator()(int r, int c) { return a[r * n + c]; }
    double operator()(int r, int c) const { return a[r * n + c]; }
};

Small small_from_colmajor(const double *m, int n)
{
    Small s;
    s.n = n;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c)
            s(r, c) = m[r + c * n];
    return s;
}

Small small_mul(const Small &x, const Small &y)
{
    Small z;
    z.n = x.n;
    for (int r = 0; r < x.n; ++r)
        for (int c = 0; c < x.n; ++c) {
            double t = 0.0;
            for (int k = 0; k < x.n; ++k)
                t += x(r, k) * y(k, c);
            z(r, c) = t;
        }
    return z;
}

// lower Cholesky factor in place; false if not positive definite
bool small_chol(Small &m)
{
    const int n = m.n;
    for (int j = 0; j < n; ++j) {
        double d = m(j, j);
        for (int k = 0; k < j; ++k)
            d -= m(j, k) * m(j, k);
        if (!(d > 0.0))
            return false;
        d = std::sqrt(d);
        m(j, j) = d;
        for (int i = j + 1; i < n; ++i) {
            double t = m(i, j);
            for (int k = 0; k < j; ++k)
                t -= m(i, k) * m(j, k);
            m(i, j) = t / d;
        }
        for (int c = j + 1; c < n; ++c)
            m(j, c) = 0.0;
    }
    return true;
}

Small small_inv_lower(const Small &L)
{
    const int n = L.n;
    Small X;
    X.n = n;
    for (int c = 0; c < n; ++c) {
        X(c, c) = 1.0 / L(c, c);
        for (int r = c + 1; r < n; ++r) {
            double t = 0.0;
            for (int k = c; k < r; ++k)
                t += L(r, k) * X(k, c);
            X(r, c) = -t / L(r, r);
        }
    }
    return X;
}

// symmetric positive definite inverse via the Cholesky factor
bool small_spd_inv(const Small &C, Small &out)
{
    Small L = C;
    if (!small_chol(L))
        return false;
    const Small Li = small_inv_lower(L);
    out.n = C.n;
    for (int r = 0; r < C.n; ++r)
        for (int c = 0; c < C.n; ++c) {
            double t = 0.0;
            for (int k = 0; k < C.n; ++k)
                t += Li(k, r) * Li(k, c);
            out(r, c) = t;
        }
    return true;
}

template <int D>
bool fill_form(GaussForm<D> &f, const double *mu, const Small &C)
{
    Small L = C;
    if (!small_chol(L))
        return false;
    const Small Li = small_inv_lower(L);
    double logdet = 0.0;
    for (int r = 0; r < D; ++r) {
        f.mu[r] = mu ? mu[r] : 0.0;
        logdet += 2.0 * std::log(L(r, r));
        for (int c = 0; c < D; ++c)
            f.linv[r * D + c] = Li(r, c);
    }
    f.logc = -0.5 * (D * LOG_2PI + logdet);
    return true;
}

Small cov_plus_w2(const Small &cov, const double *w, double cscale)
{
    Small m;
    m.n = cov.n;
    for (int r = 0; r < cov.n; ++r)
        for (int c = 0; c < cov.n; ++c)
            m(r, c) = cscale * cov(r, c) + (r == c ? w[r] * w[r] : 0.0);
    return m;
}

// The conditional covariance S - S (W + S)^-1 S, W = diag(w^2), from WSinv = (W + S)^-1, as
// W - W (W + S)^-1 W, symmetrised.  The two are equal; the first loses cov / w^2 of its digits
// where the measure is wide against the length scales (both terms are about S, the result about
// W), the second loses none there (W alone is about the result) and none where S is small.
Small cond_cov(const double *w, const Small &WSinv)
{
    const int d = WSinv.n;
    Small t;
    t.n = d;
    for (int r = 0; r < d; ++r)
        for (int c = 0; c <= r; ++c) {
            const double wr = w[r] * w[r], wc = w[c] * w[c];
            const double v = (r == c ? wr : 0.0) -
                             0.5 * ((wr * WSinv(r, c)) * wc + (wc * WSinv(c, r)) * wr);
            t(r, c) = t(c, r) = v;
        }
    return t;
}

int check_int_args(bq_ctx *c, int64_t d, const double *w, const double *mu, const double *cov)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (d < 1 || d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    if (!w || !mu || !cov)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    return BQ_OK;
}

// ---- device-side pieces shared by the host-buffer entry points and the moments ----

// out_dev[i] = scale exp(add + log N(x_i | mu, C)); with alpha_dev: *sum_dev = sum out alpha
int dev_int_K(bq_ctx *c, int d, const double *x_dev, int n, const double *mu, const Small &C,
              double scale, double add, double *out_dev, const double *alpha_dev, double *part_dev,
              double *sum_dev)
{
    const int nb = (n + 255) / 256;
    bool ok = true;
    BQ_DISPATCH_D(d, {
        GaussForm<D> f;
        ok = fill_form<D>(f, mu, C);
        if (ok)
            hipLaunchKernelGGL(int_K_kernel<D>, dim3(nb), dim3(256), 0, c->stream, x_dev, n, f,
                               scale, add, out_dev, alpha_dev, alpha_dev ? part_dev : nullptr);
    });
    if (!ok)
        return fail(c, BQ_ERR_NOT_PD, "matrix is not positive definite");
    HIPCHK(c, hipGetLastError());
    if (alpha_dev) {
        hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, c->stream, part_dev,
                           (const double *)nullptr, nb, sum_dev);
        HIPCHK(c, hipGetLastError());
    }
    return BQ_OK;
}

// C2 = [[cov + W1, cov], [cov, cov + W2]] with mean [mu, mu]
int dev_int_K1_K2(bq_ctx *c, int d, const double *x1_dev, int n1, const double *x2_dev, int n2,
                  const double *w1, const double *w2, const double *mu, const Small &cov,
                  double scale, double *out_dev, const double *alpha_dev, double *beta_dev)
{
    // The factor of C2 by blocks: L11 = chol(S + W1), L21 = S L11^-T, L22 = chol of the Schur
    // complement S + W2 - S (S + W1)^-1 S = W2 + cond_cov(W1) -- taken from C2's entries, as a
    // Cholesky sweep over all of C2 takes it, it cancels for a measure wide against w1.
    Small L11 = cov_plus_w2(cov, w1, 1.0), W1Sinv;
    if (!small_chol(L11))
        return fail(c, BQ_ERR_NOT_PD, "matrix is not positive definite");
    const Small Li11 = small_inv_lower(L11);
    W1Sinv.n = d;
    for (int r = 0; r < d; ++r)
        for (int q = 0; q < d; ++q) {
            double t = 0.0;
            for (int k = 0; k < d; ++k)
                t += Li11(k, r) * Li11(k, q);
            W1Sinv(r, q) = t;
        }
    Small L22 = cond_cov(w1, W1Sinv);
    for (int r = 0; r < d; ++r)
        L22(r, r) += w2[r] * w2[r];
    if (!small_chol(L22))
        return fail(c, BQ_ERR_NOT_PD, "matrix is not positive definite");
    const Small Li22 = small_inv_lower(L22);
    // L^-1 = [[L11^-1, 0], [-L22^-1 L21 L11^-1, L22^-1]],  L21 L11^-1 = S (S + W1)^-1
    const Small B = small_mul(Li22, small_mul(cov, W1Sinv));
    Small Linv;
    Linv.n = 2 * d;
    double mu2[MAXF], logdet = 0.0;
    for (int r = 0; r < d; ++r) {
        mu2[r] = mu2[r + d] = mu[r];
        logdet += 2.0 * (std::log(L11(r, r)) + std::log(L22(r, r)));
        for (int q = 0; q < d; ++q) {
            Linv(r, q) = Li11(r, q);
            Linv(r + d, q) = -B(r, q);
            Linv(r + d, q + d) = Li22(r, q);
        }
    }
    BQ_DISPATCH_D(d, {
        GaussForm<2 * D> f;
        for (int r = 0; r < 2 * D; ++r) {
            f.mu[r] = mu2[r];
            for (int q = 0; q < 2 * D; ++q)
                f.linv[r * 2 * D + q] = Linv(r, q);
        }
        f.logc = -0.5 * (2 * D * LOG_2PI + logdet);
        hipLaunchKernelGGL(int_K1_K2_kernel<D>, dim3((n1 + 63) / 64), dim3(256), 0, c->stream,
                           x1_dev, n1, x2_dev, n2, f, scale, out_dev, alpha_dev, beta_dev);
    });
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// int int K1 K2 K1: prepares b = G x, n1 = log N(x | mu, W1 + S) in work (d*n + n doubles)
// and either stores the n x n matrix or reduces alpha' I alpha into *sum_dev.
int dev_iikk(bq_ctx *c, int d, const double *x_dev, int n, double h1, const double *w1, double h2,
             const double *w2, const double *mu, const Small &cov, double *work_dev,
             double *out_dev, const double *alpha_dev, double *part_dev, double *sum_dev)
{
    const Small W1S = cov_plus_w2(cov, w1, 1.0);
    Small W1Sinv;
    if (!small_spd_inv(W1S, W1Sinv))
        return fail(c, BQ_ERR_NOT_PD, "matrix is not positive definite");
    const Small G = small_mul(cov, W1Sinv); // S (W1 + S)^-1
    const Small T = cond_cov(w1, W1Sinv);   // S - G S
    Small Cm;
    Cm.n = d;
    for (int r = 0; r < d; ++r)
        for (int q = 0; q < d; ++q)
            Cm(r, q) = (r == q ? w2[r] * w2[r] : 0.0) + 2.0 * T(r, q);
    double *b_dev = work_dev, *n1_dev = work_dev + (size_t)d * n;
    const double scale = (h1 * h1) * (h1 * h1) * (h2 * h2);
    const int gx = (n + 63) / 64, gy = (n + 255) / 256;
    bool ok = true;
    BQ_DISPATCH_D(d, {
        GaussForm<D> f1, g, fc;
        ok = fill_form<D>(f1, mu, W1S) && fill_form<D>(fc, nullptr, Cm);
        if (ok) {
            for (int r = 0; r < D; ++r)
                for (int q = 0; q < D; ++q)
                    g.linv[r * D + q] = G(r, q);
            hipLaunchKernelGGL(iikk_prepare_kernel<D>, dim3((n + 255) / 256), dim3(256), 0,
                               c->stream, x_dev, n, f1, g, b_dev, n1_dev);
            hipLaunchKernelGGL(int_int_K1_K2_K1_kernel<D>, dim3(gx, gy), dim3(256), 0, c->stream,
                               b_dev, n1_dev, n, fc, scale, out_dev, alpha_dev,
                               alpha_dev ? part_dev : nullptr);
        }
    });
    if (!ok)
        return fail(c, BQ_ERR_NOT_PD, "matrix is not positive definite");
    HIPCHK(c, hipGetLastError());
    if (alpha_dev) {
        hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, c->stream, part_dev,
                           (const double *)nullptr, gx * gy, sum_dev);
        HIPCHK(c, hipGetLastError());
    }
    return BQ_OK;
}

} // namespace

namespace {

// what is wrong with a measure's arrays, before any arithmetic: NULL, not finite, out of range
int check_measure(bq_ctx *c, int d, const Measure &m)
{
    if (!m.a || !m.b || (m.kind == Measure::MIX && !m.pi))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    auto finite = [](const double *v, size_t n) {
        for (size_t k = 0; k < n; ++k)
            if (!std::isfinite(v[k]))
                return false;
        return true;
    };
    switch (m.kind) {
    case Measure::GAUSS:
        if (!finite(m.a, d))
            return fail(c, BQ_ERR_BAD_ARG, "the measure's mean must be finite");
        if (!finite(m.b, (size_t)d * d))
            return fail(c, BQ_ERR_BAD_ARG, "the measure's covariance must be finite");
        return BQ_OK;
    case Measure::BOX:
        if (!finite(m.a, d) || !finite(m.b, d))
            return fail(c, BQ_ERR_BAD_ARG, "the box's ends must be finite");
        for (int k = 0; k < d; ++k)
            if (!(m.a[k] < m.b[k]))
                return fail(c, BQ_ERR_BAD_ARG, "the box needs lo < hi on every axis");
        return BQ_OK;
    case Measure::MIX: {
        if (m.C < 1 || m.C > BQ_MEASURE_MAX_COMP)
            return fail(c, BQ_ERR_BAD_ARG, "a mixture has 1..%d components", BQ_MEASURE_MAX_COMP);
        const size_t C = (size_t)m.C;
        if (!finite(m.pi, C) || !finite(m.a, C * d) || !finite(m.b, C * d * d))
            return fail(c, BQ_ERR_BAD_ARG, "the mixture's weights, means and covariances must be "
                                           "finite");
        double sum = 0.0;
        for (size_t k = 0; k < C; ++k) {
            if (m.pi[k] < 0.0)
                return fail(c, BQ_ERR_BAD_ARG, "the mixture's weights must not be negative");
            sum += m.pi[k];
        }
        if (!(sum > 0.0))
            return fail(c, BQ_ERR_BAD_ARG, "the mixture's weights sum to zero");
        return BQ_OK;
    }
    }
    return fail(c, BQ_ERR_BAD_ARG, "illegal value");
}

// -(d log 2pi + log|C|) / 2 from C's lower factor: the logc of fill_form
double form_logc(const Small &L)
{
    double logdet = 0.0;
    for (int r = 0; r < L.n; ++r)
        logdet += 2.0 * std::log(L(r, r));
    return -0.5 * (L.n * LOG_2PI + logdet);
}

// N(0 | 0, diag(w^2) + 2 cov) h^2 of a Gaussian, or BQ_ERR_BAD_ARG
int gauss_measure(bq_ctx *c, int d, double h, const double *w, const Measure &m, Small &C1,
                  double *kk)
{
    const Small S = small_from_colmajor(m.b, d);
    C1 = cov_plus_w2(S, w, 1.0);
    Small L1 = C1, L2 = cov_plus_w2(S, w, 2.0);
    if (!small_chol(L1) || !small_chol(L2))
        return fail(c, BQ_ERR_BAD_ARG,
                    "the measure's covariance plus diag(w^2) is not positive definite");
    if (kk)
        *kk = h * h * std::exp(form_logc(L2));
    return BQ_OK;
}

// h^2 prod_k I_k / L_k^2 of a box, I_k = L_k erf(L_k / (sqrt2 w_k)) + w_k sqrt(2 / pi) expm1(-L_k^2
// / (2 w_k^2)): expm1, since for a box narrow against w_k the two terms are L_k^2 sqrt(2 / pi) /
// w_k and half of it, and exp(.) - 1 would carry 1's rounding into the second
// (skip: bit k set leaves axis k out -- the kept axes of a marginal)
double box_kk(int d, double h, const double *w, const Measure &m, unsigned skip = 0)
{
    double kk = h * h;
    for (int k = 0; k < d; ++k) {
        if ((skip >> k) & 1u)
            continue;
        const double Lk = m.b[k] - m.a[k], r = Lk / (M_SQRT2 * w[k]);
        const double Ik = Lk * std::erf(r) + w[k] * std::sqrt(2.0 / M_PI) * std::expm1(-(r * r));
        kk *= Ik / (Lk * Lk);
    }
    return kk;
}

// The factors a mixture needs, or BQ_ERR_BAD_ARG: diag(w^2) + Sigma_c for every c, and with kk
// every diag(w^2) + Sigma_c + Sigma_c', over which *kk is summed in ascending c, then c'.  The
// terms (c, c') and (c', c) have the same bits -- the sum of the two covariances commutes and the
// Mahalanobis term squares the difference of the means -- so each pair is factored once.
int mix_measure(bq_ctx *c, int d, double h, const double *w, const Measure &m, double *kk)
{
    const int C = (int)m.C;
    const size_t dd = (size_t)d * d;
    for (int p = 0; p < C; ++p) {
        Small L1 = cov_plus_w2(small_from_colmajor(m.b + p * dd, d), w, 1.0);
        if (!small_chol(L1))
            return fail(c, BQ_ERR_BAD_ARG,
                        "component %d's covariance plus diag(w^2) is not positive definite", p);
    }
    if (!kk)
        return BQ_OK;
    std::vector<double> term((size_t)C * C);
    for (int p = 0; p < C; ++p)
        for (int q = p; q < C; ++q) {
            Small M;
            M.n = d;
            for (int r = 0; r < d; ++r)
                for (int s = 0; s < d; ++s)
                    M(r, s) = (m.b[p * dd + r + s * d] + m.b[q * dd + r + s * d]) +
                              (r == s ? w[r] * w[r] : 0.0);
            if (!small_chol(M))
                return fail(c, BQ_ERR_BAD_ARG,
                            "the covariances of components %d and %d plus diag(w^2) are not "
                            "positive definite", p, q);
            const Small Li = small_inv_lower(M);
            double maha = 0.0;
            for (int r = 0; r < d; ++r) {
                double y = 0.0;
                for (int s = 0; s <= r; ++s)
                    y += Li(r, s) * (m.a[s + (size_t)p * d] - m.a[s + (size_t)q * d]);
                maha += y * y;
            }
            term[(size_t)p * C + q] = term[(size_t)q * C + p] =
                h * h * std::exp(form_logc(M) - 0.5 * maha);
        }
    double sum = 0.0;
    for (int p = 0; p < C; ++p)
        for (int q = 0; q < C; ++q) {
            const double t = m.pi[p] * m.pi[q] * term[(size_t)p * C + q];
            sum = (p | q) ? sum + t : t;
        }
    *kk = sum;
    return BQ_OK;
}

} // namespace

// the forms of a legal mixture as int_K_mix_kernel reads them (host.h; fit.hip, kmean_enqueue)
void bqh::mix_forms(int d, const double *w, const Measure &m, double *host)
{
    const int C = (int)m.C;
    BQ_DISPATCH_D(d, {
        GaussForm<D> *f = reinterpret_cast<GaussForm<D> *>(host);
        for (int p = 0; p < C; ++p)
            (void)fill_form<D>(f[p], m.a + (size_t)p * D,
                               cov_plus_w2(small_from_colmajor(m.b + (size_t)p * D * D, D), w, 1.0));
        std::memcpy(f + C, m.pi, sizeof(double) * C);
    });
}

// the kernel mean of a measure at device points and the prior variance of the integral
// (host.h; fit.hip, kmean_enqueue and the designs' bodies)
int bqh::launch_kernel_mean(bq_ctx *c, int d, const double *x, int n, double h, const double *w,
                            const Measure &m, double *out, double *kk, const double *forms)
{
    BQCHK(check_measure(c, d, m));
    const int nb = (n + 255) / 256;
    // (the launch profiler's row of a kernel mean: the points read and the values written)
    const double work = 8.0 * (d + 1.0) * n;
    switch (m.kind) {
    case Measure::GAUSS: {
        Small C1;
        BQCHK(gauss_measure(c, d, h, w, m, C1, kk));
        if (n == 0)
            return BQ_OK;
        Bracket br(c, BQ_K_REDUCE, work);
        return dev_int_K(c, d, x, n, m.a, C1, h * h, 0.0, out, nullptr, nullptr, nullptr);
    }
    case Measure::BOX: {
        if (kk)
            *kk = box_kk(d, h, w, m);
        if (n == 0)
            return BQ_OK;
        Bracket br(c, BQ_K_REDUCE, work);
        BQ_DISPATCH_D(d, {
            BoxForm<D> f;
            for (int k = 0; k < D; ++k) {
                f.lo[k] = m.a[k], f.hi[k] = m.b[k];
                f.rw[k] = 1.0 / (M_SQRT2 * w[k]), f.rl[k] = 1.0 / (m.b[k] - m.a[k]);
            }
            hipLaunchKernelGGL(int_K_box_kernel<D>, dim3(nb), dim3(256), 0, c->stream, x, n, f,
                               h * h, out);
        });
        break;
    }
    case Measure::MIX: {
        BQCHK(mix_measure(c, d, h, w, m, kk));
        if (n == 0)
            return BQ_OK;
        if (!forms)
            return fail(c, BQ_ERR_BAD_ARG, "a mixture's forms are not on the device");
        Bracket br(c, BQ_K_REDUCE, work);
        BQ_DISPATCH_D(d, {
            const GaussForm<D> *f = reinterpret_cast<const GaussForm<D> *>(forms);
            hipLaunchKernelGGL(int_K_mix_kernel<D>, dim3(nb), dim3(256), 0, c->stream, x, n, f,
                               reinterpret_cast<const double *>(f + m.C), (int)m.C, h * h, out);
        });
        break;
    }
    }
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// the transforms and constants of square-root-warped quadrature (host.h; types.h, SqForms; fit.hip,
// bq_gp_sqintegral and bq_gp_sqdesign).  With Lambda = diag(w^2), S = cov:
//   W(p, q) = h^4 N(p - q | 0, 2 Lambda) N((p + q) / 2 | mu, Lambda / 2 + S)
//   Q_ij    = h^6 n_i n_j N(G (x_i - x_j) | 0, Lambda + 2 S - 2 G S),  G = S (Lambda + S)^-1,
//             n = N(x | mu, Lambda + S)          (dev_iikk's algebra with K1 = K2)
int bqh::sq_forms(bq_ctx *c, int d, double h, const double *w, const double *mu, const double *cov,
                  SqForms *out)
{
    for (int k = 0; k < d; ++k)
        if (!std::isfinite(mu[k]))
            return fail(c, BQ_ERR_BAD_ARG, "the measure's mean must be finite");
    for (int k = 0; k < d * d; ++k)
        if (!std::isfinite(cov[k]))
            return fail(c, BQ_ERR_BAD_ARG, "the measure's covariance must be finite");
    const Small S = small_from_colmajor(cov, d);
    const Small C1 = cov_plus_w2(S, w, 1.0);
    Small L1 = C1, L2 = cov_plus_w2(S, w, 2.0), C1inv;
    for (int k = 0; k < d * d; ++k)
        L2.a[k] *= 0.5; // Lambda / 2 + S
    if (!small_chol(L1) || !small_chol(L2) || !small_spd_inv(C1, C1inv))
        return fail(c, BQ_ERR_BAD_ARG,
                    "the measure's covariance plus diag(w^2) is not positive definite");
    const Small G = small_mul(S, C1inv), T = cond_cov(w, C1inv); // T = S - G S
    Small L3;
    L3.n = d;
    for (int r = 0; r < d; ++r)
        for (int q = 0; q < d; ++q)
            L3(r, q) = (r == q ? w[r] * w[r] : 0.0) + 2.0 * T(r, q);
    if (!small_chol(L3))
        return fail(c, BQ_ERR_BAD_ARG,
                    "the measure's covariance gives no positive definite diag(w^2) + 2 (diag(w^-2) "
                    "+ cov^-1)^-1");
    const Small Li1 = small_inv_lower(L1), Li2 = small_inv_lower(L2);
    const Small A3 = small_mul(small_inv_lower(L3), G);
    SqForms f{};
    double ld1 = 0.0, ld2 = 0.0, ld3 = 0.0, ldw = 0.0;
    for (int r = 0; r < d; ++r) {
        ld1 += 2.0 * std::log(L1(r, r));
        ld2 += 2.0 * std::log(L2(r, r));
        ld3 += 2.0 * std::log(L3(r, r));
        ldw += std::log(2.0 * w[r] * w[r]);
        f.mu[r] = mu[r];
        f.a1w[r * d + r] = 1.0 / (std::sqrt(2.0) * w[r]);
        for (int q = 0; q < d; ++q) {
            f.a2w[r * d + q] = 0.5 * Li2(r, q);
            f.kl[r * d + q] = Li1(r, q);
            f.a1q[r * d + q] = A3(r, q);
        }
    }
    const double h2 = h * h;
    f.klogc = -0.5 * (d * LOG_2PI + ld1);
    f.cw = h2 * h2 * std::exp(-0.5 * (d * LOG_2PI + ldw) - 0.5 * (d * LOG_2PI + ld2));
    f.cq = h2 * h2 * h2 * std::exp(-0.5 * (d * LOG_2PI + ld3));
    *out = f;
    return BQ_OK;
}

// the plan of a marginal (host.h, MargPlan; marginal.h has the expression the numbers enter)
int bqh::marginal_plan(bq_ctx *c, int d, double h, const double *w, const int32_t *keep,
                       const Measure &m, const double *xq, int64_t M, MargPlan *out)
{
    BQCHK(launch_kernel_mean(c, d, nullptr, 0, h, w, m, nullptr, nullptr));
    if (m.kind == Measure::MIX)
        return fail(c, BQ_ERR_BAD_ARG, "a mixture has no marginal here");
    if (!keep)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    MargPlan p;
    p.d = d, p.box = m.kind == Measure::BOX, p.h2 = h * h;
    int S[BQ_MAXD], I[BQ_MAXD], ns = 0, ni = 0;
    for (int k = 0; k < d; ++k) {
        if (keep[k] != 0 && keep[k] != 1)
            return fail(c, BQ_ERR_BAD_ARG, "a keep flag is 0 or 1");
        if (keep[k])
            S[ns++] = k, p.keep |= 1u << k;
        else
            I[ni++] = k;
    }
    if (ns == 0 || ni == 0)
        return fail(c, BQ_ERR_BAD_ARG, "a marginal keeps between 1 and d - 1 axes");
    if (xq)
        for (int64_t j = 0; j < M; ++j)
            for (int a = 0; a < ns; ++a)
                if (!std::isfinite(xq[S[a] + j * d]))
                    return fail(c, BQ_ERR_BAD_ARG, "a kept coordinate of a query point is not finite");
    const double inf = std::numeric_limits<double>::infinity();
    double lcS = 0.0; // log N(0 | 0, W_S)
    for (int k = 0; k < BQ_MAXD; ++k) {
        p.lo[k] = p.ilo[k] = -inf, p.hi[k] = p.ihi[k] = inf;
        p.rl[k] = 1.0, p.rw[k] = k < d ? 1.0 / (M_SQRT2 * w[k]) : 1.0;
    }
    for (int a = 0; a < ns; ++a) {
        const int k = S[a];
        lcS += -0.5 * LOG_2PI - std::log(w[k]);
        p.le[k * d + k] = p.g[k * d + k] = 1.0 / w[k];
    }
    if (p.box) {
        double vol = 1.0;
        for (int a = 0; a < ns; ++a) {
            p.lo[S[a]] = m.a[S[a]], p.hi[S[a]] = m.b[S[a]];
            vol *= m.b[S[a]] - m.a[S[a]];
        }
        for (int i = 0; i < ni; ++i) {
            p.ilo[I[i]] = m.a[I[i]], p.ihi[I[i]] = m.b[I[i]];
            p.rl[I[i]] = 1.0 / (m.b[I[i]] - m.a[I[i]]);
        }
        p.rvol = 1.0 / vol;
        p.scale_e = p.rvol, p.logc_e = lcS;
        p.scale_p = box_kk(d, h, w, m, p.keep), p.logc_p = lcS;
        *out = p;
        return BQ_OK;
    }
    const double *cov = m.b;
    for (int r = 0; r < d; ++r)
        for (int q = 0; q < r; ++q) {
            const double u = cov[r + q * d], v = cov[q + r * d];
            if (std::fabs(u - v) > 1e-12 * std::max(std::fabs(u), std::fabs(v)))
                return fail(c, BQ_ERR_BAD_ARG, "the measure's covariance must be symmetric");
        }
    Small Lss;
    Lss.n = ns;
    for (int a = 0; a < ns; ++a)
        for (int b = 0; b < ns; ++b)
            Lss(a, b) = cov[S[a] + S[b] * d];
    if (!small_chol(Lss))
        return fail(c, BQ_ERR_BAD_ARG,
                    "the measure's covariance is not positive definite on the kept axes");
    const Small Li = small_inv_lower(Lss);
    p.lq = form_logc(Lss);
    double B[BQ_MAXD][BQ_MAXD] = {{0}};
    for (int a = 0; a < ns; ++a)
        for (int b = 0; b <= a; ++b)
            p.ls[S[a] * d + S[b]] = Li(a, b);
    for (int i = 0; i < ni; ++i)
        for (int a = 0; a < ns; ++a) {
            double t = 0.0;
            for (int b = 0; b < ns; ++b) {
                double inv = 0.0; // (Sigma_SS^-1)(b, a)
                for (int k = 0; k < ns; ++k)
                    inv += Li(k, b) * Li(k, a);
                t += cov[I[i] + S[b] * d] * inv;
            }
            B[i][a] = t;
            p.bm[I[i] * d + S[a]] = t;
        }
    Small E1, E2;
    E1.n = E2.n = ni;
    for (int i = 0; i < ni; ++i)
        for (int j = 0; j <= i; ++j) {
            double t = 0.0, u = 0.0;
            for (int a = 0; a < ns; ++a) {
                t += B[i][a] * cov[S[a] + I[j] * d];
                u += B[j][a] * cov[S[a] + I[i] * d];
            }
            const double sc = cov[I[i] + I[j] * d] - 0.5 * (t + u); // Sigma_c, symmetrised
            const double wi = i == j ? w[I[i]] * w[I[i]] : 0.0;
            E1(i, j) = E1(j, i) = wi + sc;
            E2(i, j) = E2(j, i) = wi + 2.0 * sc;
        }
    if (!small_chol(E1) || !small_chol(E2))
        return fail(c, BQ_ERR_BAD_ARG, "the conditional covariance of the integrated axes plus "
                                       "diag(w^2) is not positive definite");
    const Small Li1 = small_inv_lower(E1), Li2 = small_inv_lower(E2);
    for (int i = 0; i < ni; ++i) {
        for (int j = 0; j <= i; ++j)
            p.le[I[i] * d + I[j]] = Li1(i, j);
        for (int a = 0; a < ns; ++a) {
            double t = 0.0;
            for (int j = 0; j <= i; ++j)
                t += Li2(i, j) * B[j][a];
            p.g[I[i] * d + S[a]] = t;
        }
    }
    for (int k = 0; k < d; ++k)
        p.mu[k] = m.a[k];
    p.scale_e = p.scale_p = h * h;
    p.logc_e = lcS + form_logc(E1);
    p.logc_p = lcS + form_logc(E2);
    *out = p;
    return BQ_OK;
}

namespace {

template <int D>
MargForm<D> marg_form(const MargPlan &p)
{
    MargForm<D> f;
    for (int r = 0; r < D; ++r) {
        f.mu[r] = p.mu[r], f.lo[r] = p.lo[r], f.hi[r] = p.hi[r];
        for (int q = 0; q < D; ++q) {
            f.ls[r * D + q] = p.ls[r * D + q];
            f.bm[r * D + q] = p.bm[r * D + q];
            f.le[r * D + q] = p.le[r * D + q];
        }
    }
    f.lq = p.lq, f.logc = p.logc_e, f.scale = p.scale_e, f.keep = p.keep;
    return f;
}

} // namespace

int bqh::launch_marginal_colv(bq_ctx *c, const MargPlan &pl, const double *x, int n, double *colv)
{
    Bracket br(c, BQ_K_REDUCE, 8.0 * (pl.d + 1.0) * n);
    BQ_DISPATCH_D(pl.d, {
        BoxForm<D> f;
        for (int k = 0; k < D; ++k)
            f.lo[k] = pl.ilo[k], f.hi[k] = pl.ihi[k], f.rw[k] = pl.rw[k], f.rl[k] = pl.rl[k];
        hipLaunchKernelGGL(int_K_box_kernel<D>, dim3((n + 255) / 256), dim3(256), 0, c->stream, x, n,
                           f, pl.h2, colv);
    });
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int bqh::launch_marginal_cross(bq_ctx *c, const MargPlan &pl, const double *xq, int M, int Mp,
                               const double *x, int n, int npad, const double *colv, double *K,
                               long ldk)
{
    if (M < 1 || n < 1 || Mp % 64 || npad % 64 || Mp < M || npad < n || ldk < Mp)
        return fail(c, BQ_ERR_BAD_ARG, "marginal_cross: padded sizes must be multiples of 64");
    Bracket br(c, BQ_K_GRAM, 8.0 * Mp * npad);
    const dim3 grid(Mp / 64, npad / 64);
    BQ_DISPATCH_D(pl.d, {
        const MargForm<D> f = marg_form<D>(pl);
        if (pl.box)
            hipLaunchKernelGGL((marginal_cross_kernel<D, true>), grid, dim3(256), 0, c->stream, xq, M,
                               x, n, f, colv, K, ldk);
        else
            hipLaunchKernelGGL((marginal_cross_kernel<D, false>), grid, dim3(256), 0, c->stream, xq,
                               M, x, n, f, colv, K, ldk);
    });
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int bqh::launch_marginal_mean(bq_ctx *c, const MargPlan &pl, const double *xq, int M,
                              const double *x, int n, const double *colv, const double *alpha,
                              double *mean)
{
    Bracket br(c, BQ_K_REDUCE);
    const dim3 grid((unsigned)((M + 3) / 4));
    BQ_DISPATCH_D(pl.d, {
        const MargForm<D> f = marg_form<D>(pl);
        if (pl.box)
            hipLaunchKernelGGL((marginal_mean_kernel<D, true>), grid, dim3(256), 0, c->stream, xq, M,
                               x, n, f, colv, alpha, mean);
        else
            hipLaunchKernelGGL((marginal_mean_kernel<D, false>), grid, dim3(256), 0, c->stream, xq,
                               M, x, n, f, colv, alpha, mean);
    });
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

int bqh::launch_marginal_prior(bq_ctx *c, const MargPlan &pl, const double *xq, int M, int Mp,
                               double *P, long ldp, double *diag, int accum)
{
    if (M < 1 || Mp % 64 || Mp < M || (P && ldp < Mp) || (!P && !diag))
        return fail(c, BQ_ERR_BAD_ARG, "marginal_prior: the padded size must be a multiple of 64");
    Bracket br(c, BQ_K_GRAM, P ? 8.0 * Mp * Mp : 8.0 * M);
    const dim3 grid(Mp / 64, P ? Mp / 64 : 1);
    BQ_DISPATCH_D(pl.d, {
        MargPrior<D> f;
        for (int r = 0; r < D; ++r) {
            f.mu[r] = pl.mu[r], f.lo[r] = pl.lo[r], f.hi[r] = pl.hi[r];
            for (int q = 0; q < D; ++q)
                f.ls[r * D + q] = pl.ls[r * D + q], f.g[r * D + q] = pl.g[r * D + q];
        }
        f.lq = pl.lq, f.logc = pl.logc_p, f.scale = pl.scale_p, f.rvol = pl.rvol, f.keep = pl.keep;
        hipLaunchKernelGGL(marginal_prior_kernel<D>, grid, dim3(256), 0, c->stream, xq, M, f, P, ldp,
                           diag, accum);
    });
    HIPCHK(c, hipGetLastError());
    return BQ_OK;
}

// ===========================================================================
// gauss_c drop-ins: host buffers in and out
// ===========================================================================
extern "C" int bq_int_K(bq_ctx *c, const double *x, int64_t d, int64_t n, double h, const double *w,
                        const double *mu, const double *cov, double *out)
{
    BQCHK(check_int_args(c, d, w, mu, cov));
    if (n < 0 || (n && (!x || !out)))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (n == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf xd, od;
    HIPCHK(c, xd.alloc(sizeof(double) * d * n));
    HIPCHK(c, od.alloc(sizeof(double) * n));
    HIPCHK(c, hipMemcpyAsync(xd.p, x, sizeof(double) * d * n, hipMemcpyHostToDevice, c->stream));
    const Small S = small_from_colmajor(cov, (int)d);
    BQCHK(dev_int_K(c, (int)d, xd.d(), (int)n, mu, cov_plus_w2(S, w, 1.0), h * h, 0.0, od.d(),
                    nullptr, nullptr, nullptr));
    HIPCHK(c, hipMemcpyAsync(out, od.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

namespace {

// bq_int_K_box and bq_int_K_mix: kappa at n host points, kk on the host
int int_K_measure(bq_ctx *c, const double *x, int64_t d, int64_t n, double h, const double *w,
                  const Measure &m, double *out, double *kk)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (d < 1 || d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    if (!w || n < 0 || n > INT32_MAX || (!out && !kk) || (out && n && !x))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    // (the measure is checked, with the factors that only kk needs, before anything is allocated)
    double kk0 = 0.0;
    BQCHK(launch_kernel_mean(c, (int)d, nullptr, 0, h, w, m, nullptr, kk ? &kk0 : nullptr));
    if (!out || n == 0) {
        if (kk)
            *kk = kk0;
        return BQ_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf xd, od, fd;
    std::vector<double> hf;
    HIPCHK(c, xd.alloc(sizeof(double) * d * n));
    HIPCHK(c, od.alloc(sizeof(double) * n));
    HIPCHK(c, hipMemcpyAsync(xd.p, x, sizeof(double) * d * n, hipMemcpyHostToDevice, c->stream));
    if (m.kind == Measure::MIX) {
        hf.resize(mix_form_doubles((int)d, (int)m.C));
        HIPCHK(c, fd.alloc(sizeof(double) * hf.size()));
        mix_forms((int)d, w, m, hf.data());
        HIPCHK(c, hipMemcpyAsync(fd.p, hf.data(), sizeof(double) * hf.size(),
                                 hipMemcpyHostToDevice, c->stream));
    }
    const int st = launch_kernel_mean(c, (int)d, xd.d(), (int)n, h, w, m, od.d(), nullptr, fd.d());
    if (st == BQ_OK)
        (void)hipMemcpyAsync(out, od.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (x, hf and the buffers are read until here)
    HIPCHK(c, hipGetLastError());
    if (st == BQ_OK && kk)
        *kk = kk0;
    return st;
}

} // namespace

extern "C" int bq_int_K_box(bq_ctx *c, const double *x, int64_t d, int64_t n, double h,
                            const double *w, const double *lo, const double *hi, double *out,
                            double *kk)
{
    return int_K_measure(c, x, d, n, h, w, Measure::box(lo, hi), out, kk);
}

extern "C" int bq_int_K_mix(bq_ctx *c, const double *x, int64_t d, int64_t n, double h,
                            const double *w, int64_t C, const double *pi, const double *mu,
                            const double *cov, double *out, double *kk)
{
    return int_K_measure(c, x, d, n, h, w, Measure::mix(C, pi, mu, cov), out, kk);
}

namespace {

// bq_marginal_K and bq_marginal_K_box: the cross matrix c(xq, x), M x n, and the prior's diagonal
// at host points without a fit, through the kernels bq_gp_marginal runs
int marginal_K(bq_ctx *c, const double *xq, int64_t M, const double *x, int64_t n, int64_t d,
               double h, const double *w, const int32_t *keep, const Measure &m, double *out,
               double *pdiag)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (d < 1 || d > BQ_MAXD)
        return fail(c, BQ_ERR_BAD_ARG, "d must be in 1..%d", BQ_MAXD);
    BQCHK(check_w(c, d, h, w, 0.0));
    if (M < 0 || n < 0 || M > INT32_MAX - 64 || n > INT32_MAX - 64 || (!out && !pdiag) ||
        (M && !xq) || (out && M && n && !x))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    MargPlan pl;
    BQCHK(marginal_plan(c, (int)d, h, w, keep, m, xq, M, &pl));
    if (M == 0)
        return BQ_OK;
    const bool cross = out && n;
    const int Mp = (int)roundup(M, 64), npad = (int)roundup(n, 64);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf qd, xd, Kd, cd, dd;
    HIPCHK(c, qd.alloc(sizeof(double) * d * M));
    HIPCHK(c, dd.alloc(sizeof(double) * M));
    if (cross) {
        HIPCHK(c, xd.alloc(sizeof(double) * d * n));
        HIPCHK(c, Kd.alloc(sizeof(double) * (size_t)Mp * npad));
        HIPCHK(c, cd.alloc(sizeof(double) * npad));
    }
    HIPCHK(c, hipMemcpyAsync(qd.p, xq, sizeof(double) * d * M, hipMemcpyHostToDevice, c->stream));
    int st = BQ_OK;
    if (cross) {
        HIPCHK(c, hipMemcpyAsync(xd.p, x, sizeof(double) * d * n, hipMemcpyHostToDevice, c->stream));
        if (pl.box)
            st = launch_marginal_colv(c, pl, xd.d(), (int)n, cd.d());
        if (st == BQ_OK)
            st = launch_marginal_cross(c, pl, qd.d(), (int)M, Mp, xd.d(), (int)n, npad, cd.d(),
                                       Kd.d(), Mp);
        if (st == BQ_OK)
            (void)hipMemcpy2DAsync(out, sizeof(double) * M, Kd.p, sizeof(double) * Mp,
                                   sizeof(double) * M, n, hipMemcpyDeviceToHost, c->stream);
    }
    if (st == BQ_OK && pdiag) {
        st = launch_marginal_prior(c, pl, qd.d(), (int)M, Mp, nullptr, 0, dd.d(), 0);
        if (st == BQ_OK)
            (void)hipMemcpyAsync(pdiag, dd.p, sizeof(double) * M, hipMemcpyDeviceToHost, c->stream);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the host arrays and the buffers are read until here)
    HIPCHK(c, hipGetLastError());
    return st;
}

} // namespace

extern "C" int bq_marginal_K(bq_ctx *c, const double *xq, int64_t M, const double *x, int64_t n,
                             int64_t d, double h, const double *w, const int32_t *keep,
                             const double *mu, const double *cov, double *out, double *pdiag)
{
    return marginal_K(c, xq, M, x, n, d, h, w, keep, Measure::gauss(mu, cov), out, pdiag);
}

extern "C" int bq_marginal_K_box(bq_ctx *c, const double *xq, int64_t M, const double *x, int64_t n,
                                 int64_t d, double h, const double *w, const int32_t *keep,
                                 const double *lo, const double *hi, double *out, double *pdiag)
{
    return marginal_K(c, xq, M, x, n, d, h, w, keep, Measure::box(lo, hi), out, pdiag);
}

extern "C" int bq_int_K1_K2(bq_ctx *c, const double *x1, int64_t n1, const double *x2, int64_t n2,
                            int64_t d, double h1, const double *w1, double h2, const double *w2,
                            const double *mu, const double *cov, double *out)
{
    BQCHK(check_int_args(c, d, w1, mu, cov));
    if (!w2 || n1 < 0 || n2 < 0 || (n1 && !x1) || (n2 && !x2) || (n1 * n2 && !out))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (n1 == 0 || n2 == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf a, b, od;
    HIPCHK(c, a.alloc(sizeof(double) * d * n1));
    HIPCHK(c, b.alloc(sizeof(double) * d * n2));
    HIPCHK(c, od.alloc(sizeof(double) * (size_t)n1 * n2));
    HIPCHK(c, hipMemcpyAsync(a.p, x1, sizeof(double) * d * n1, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.p, x2, sizeof(double) * d * n2, hipMemcpyHostToDevice, c->stream));
    const Small S = small_from_colmajor(cov, (int)d);
    BQCHK(dev_int_K1_K2(c, (int)d, a.d(), (int)n1, b.d(), (int)n2, w1, w2, mu, S,
                        (h1 * h1) * (h2 * h2), od.d(), nullptr, nullptr));
    HIPCHK(c, hipMemcpyAsync(out, od.p, sizeof(double) * (size_t)n1 * n2, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

extern "C" int bq_int_int_K1_K2_K1(bq_ctx *c, const double *x, int64_t d, int64_t n, double h1,
                                   const double *w1, double h2, const double *w2, const double *mu,
                                   const double *cov, double *out)
{
    BQCHK(check_int_args(c, d, w1, mu, cov));
    if (!w2 || n < 0 || (n && (!x || !out)))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (n == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf xd, wk, od;
    HIPCHK(c, xd.alloc(sizeof(double) * d * n));
    HIPCHK(c, wk.alloc(sizeof(double) * (d + 1) * n));
    HIPCHK(c, od.alloc(sizeof(double) * (size_t)n * n));
    HIPCHK(c, hipMemcpyAsync(xd.p, x, sizeof(double) * d * n, hipMemcpyHostToDevice, c->stream));
    const Small S = small_from_colmajor(cov, (int)d);
    BQCHK(dev_iikk(c, (int)d, xd.d(), (int)n, h1, w1, h2, w2, mu, S, wk.d(), od.d(), nullptr,
                   nullptr, nullptr));
    HIPCHK(c, hipMemcpyAsync(out, od.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

extern "C" int bq_int_int_K1_K2(bq_ctx *c, const double *x, int64_t d, int64_t n, double h1,
                                const double *w1, double h2, const double *w2, const double *mu,
                                const double *cov, double *out)
{
    BQCHK(check_int_args(c, d, w1, mu, cov));
    if (!w2 || n < 0 || (n && (!x || !out)))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (n == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const Small S = small_from_colmajor(cov, (int)d);
    const Small W = cov_plus_w2(S, w1, 2.0);
    Small Wl = W, Winv;
    if (!small_chol(Wl) || !small_spd_inv(W, Winv))
        return fail(c, BQ_ERR_NOT_PD, "matrix is not positive definite");
    double logdet = 0.0;
    for (int r = 0; r < d; ++r)
        logdet += 2.0 * std::log(Wl(r, r));
    const double N0 = -0.5 * (d * LOG_2PI + logdet); // log N(0 | 0, W1 + 2S)
    const Small SWS = small_mul(small_mul(S, Winv), S);
    Small Cm;
    Cm.n = (int)d;
    for (int r = 0; r < d; ++r)
        for (int q = 0; q < d; ++q)
            Cm(r, q) = (r == q ? w2[r] * w2[r] : 0.0) + S(r, q) - SWS(r, q);
    DevBuf xd, od;
    HIPCHK(c, xd.alloc(sizeof(double) * d * n));
    HIPCHK(c, od.alloc(sizeof(double) * n));
    HIPCHK(c, hipMemcpyAsync(xd.p, x, sizeof(double) * d * n, hipMemcpyHostToDevice, c->stream));
    BQCHK(dev_int_K(c, (int)d, xd.d(), (int)n, mu, Cm, (h1 * h1) * (h2 * h2), N0, od.d(), nullptr,
                    nullptr, nullptr));
    HIPCHK(c, hipMemcpyAsync(out, od.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// ===========================================================================
// resident-factor solve and the BQ moments on device-resident fits
// ===========================================================================
extern "C" int bq_gp_solve(bq_ctx *c, bq_fit *f, const double *B, int64_t nrhs, double *X)
{
    BQCHK(check_fit(c, f));
    if (nrhs < 0 || (nrhs && (!B || !X)))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (nrhs == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const int n = f->n, npad = f->npad;
    if (nrhs == 1) {
        // one right-hand side: the GEMV sweeps (trsv.h)
        WideInv wv;
        BQCHK(fit_wide(c, f, wv));
        BQCHK(fit_vec(c, f));
        double *x = f->vec.d(), *y = f->vec.d() + npad;
        // (a timed-out hand-off of the one-launch sweeps re-issues the solve on the per-block
        // kernels: with_flow_fallback)
        BQCHK(with_flow_fallback(c, [&]() -> int {
            // through the fit's pinned staging vector (zero padded): truly asynchronous copies
            std::memcpy(f->hvec, B, sizeof(double) * n);
            std::memset(f->hvec + n, 0, sizeof(double) * (npad - n));
            if (c->cfg.solve_kcopy && trsv_flow_ok(c, npad, wv.B, true)) {
                // [x | y | ws_f | x_out | ws_b]: the vector comes in and goes out through kernels
                // on the mapped pinned vector, and one of them sets both sweeps' hand-off slots
                double *hdev = nullptr;
                HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&hdev), f->hvec, 0));
                const size_t wsn = trsv_flow_ws_doubles(npad, wv.B);
                double *wsf = y + npad, *xo = wsf + wsn, *wsb = xo + npad;
                BQCHK(launch_flow_in(c, hdev, n, x, npad, y, 2 * (size_t)npad + 2 * wsn));
                BQCHK(launch_trsv_flow(c, true, f->A.d(), f->ldl, npad, wv.B, wv.nr, wv.tt, x, y,
                                       wsf, true));
                BQCHK(launch_trsv_flow(c, false, f->A.d(), f->ldl, npad, wv.B, wv.nt, wv.uu, y, xo,
                                       wsb, true));
                BQCHK(launch_flow_out(c, xo, n, hdev));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                return BQ_OK;
            }
            double *hmap = nullptr;
            if (c->cfg.solve_kcopy)
                HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void **>(&hmap), f->hvec, 0));
            if (hmap)
                BQCHK(launch_flow_in(c, hmap, n, x, npad, nullptr, 0));
            else
                HIPCHK(c, hipMemcpyAsync(x, f->hvec, sizeof(double) * npad, hipMemcpyHostToDevice,
                                         c->stream));
            BQCHK(fit_replay(c, f, 0, [&]() -> int {
                double *ws = f->vec.d() + 2 * (size_t)npad;
                BQCHK(enqueue_forward_vec(c, x, y, f->A.d(), f->ldl, npad, wv, ws));
                return enqueue_backward_vec(c, y, x, f->A.d(), f->ldl, npad, wv, ws);
            }));
            if (hmap)
                BQCHK(launch_flow_out(c, x, n, hmap));
            else
                HIPCHK(c, hipMemcpyAsync(f->hvec, x, sizeof(double) * n, hipMemcpyDeviceToHost,
                                         c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return BQ_OK;
        }));
        std::memcpy(X, f->hvec, sizeof(double) * n);
        return BQ_OK;
    }
    WideInv wi;
    BQCHK(fit_wide(c, f, wi));
    return solve_rows_host(c, f->A.d(), f->ldl, n, npad, wi, B, nrhs, X);
}

extern "C" int bq_bq_Z_mean(bq_ctx *c, bq_fit *gp_l, const double *mu, const double *cov,
                            double *out)
{
    BQCHK(check_fit(c, gp_l));
    if (!out)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    BQCHK(check_int_args(c, gp_l->d, gp_l->w, mu, cov));
    HIPCHK(c, hipSetDevice(c->device));
    BQCHK(fit_alpha(c, gp_l));
    const int d = gp_l->d, n = gp_l->n;
    Scratch sc(c);
    const size_t opart = sc.take((size_t)(n + 255) / 256 + 1);
    BQCHK(sc.commit());
    double *part = sc.at(opart);
    const Small S = small_from_colmajor(cov, d);
    double *sum_dev = part + (n + 255) / 256;
    BQCHK(dev_int_K(c, d, gp_l->pts.d(), n, mu, cov_plus_w2(S, gp_l->w, 1.0), gp_l->h * gp_l->h,
                    0.0, nullptr, gp_l->alpha.d(), part, sum_dev));
    HIPCHK(c, hipMemcpyAsync(out, sum_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BQ_OK;
}

extern "C" int bq_bq_Z_var(bq_ctx *c, bq_fit *gp_tl, bq_fit *gp_l, const double *mu,
                           const double *cov, double *out)
{
    BQCHK(check_fit(c, gp_tl));
    BQCHK(check_fit(c, gp_l));
    if (!out)
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (gp_tl->d != gp_l->d)
        return fail(c, BQ_ERR_BAD_ARG, "dimension mismatch");
    BQCHK(check_int_args(c, gp_l->d, gp_l->w, mu, cov));
    HIPCHK(c, hipSetDevice(c->device));
    BQCHK(fit_alpha(c, gp_l));
    const int d = gp_l->d, ns = gp_tl->n, nsc = gp_l->n, npad = gp_tl->npad;
    const Small S = small_from_colmajor(cov, d);
    const int gx = (nsc + 63) / 64, gy = (nsc + 255) / 256;
    WideInv wi;
    BQCHK(fit_wide(c, gp_tl, wi));
    Scratch sc(c);
    const size_t owork = sc.take((size_t)(d + 1) * nsc), opart = sc.take((size_t)gx * gy + 4);
    BQCHK(sc.commit());
    double *work = sc.at(owork), *part = sc.at(opart);
    BQCHK(fit_vec(c, gp_tl));
    double *sol = gp_tl->vec.d(), *X = gp_tl->vec.d() + npad;
    double *scal = part + (size_t)gx * gy; // [0] = alpha' I alpha, [1] = -beta' K^-1 beta
    // alpha' (int int K_l K_tl K_l) alpha
    BQCHK(dev_iikk(c, d, gp_l->pts.d(), nsc, gp_l->h, gp_l->w, gp_tl->h, gp_tl->w, mu, S, work,
                   nullptr, gp_l->alpha.d(), part, scal));
    double hs[2];
    BQCHK(with_flow_fallback(c, [&]() -> int {
        // beta = (int K_tl K_l) alpha
        HIPCHK(c, hipMemsetAsync(sol, 0, sizeof(double) * (size_t)npad, c->stream));
        BQCHK(dev_int_K1_K2(c, d, gp_tl->pts.d(), ns, gp_l->pts.d(), nsc, gp_tl->w, gp_l->w, mu, S,
                            (gp_tl->h * gp_tl->h) * (gp_l->h * gp_l->h), nullptr, gp_l->alpha.d(),
                            sol));
        // beta' K_tl^-1 beta = |L_tl^-1 beta|^2: the forward sweep alone and a sum of squares
        // (the reference solves with both sweeps and takes the dot product, bq_c.pyx:348-351; the
        // symmetric form errs with cond(L) instead of cond(K))
        BQCHK(fit_replay(c, gp_tl, 2, [&]() -> int {
            return enqueue_forward_vec(c, sol, X, gp_tl->A.d(), gp_tl->ldl, npad, wi,
                                       gp_tl->vec.d() + 2 * (size_t)npad);
        }));
        BQCHK(launch_neg_sumsq(c, X, npad, scal + 1));
        HIPCHK(c, hipMemcpyAsync(hs, scal, sizeof hs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BQ_OK;
    }));
    *out = hs[0] + hs[1]; // hs[1] holds -|L^-1 beta|^2
    return BQ_OK;
}

// ===========================================================================
// batched expected-squared-mean systems
// ===========================================================================
extern "C" int bq_esm_batch(bq_ctx *c, const double *x_sc, const double *l_sc, int64_t ns,
                            int64_t nsc, const double *x_a, int64_t M, double h, double w,
                            double thresh, const double *mu, const double *cov, double *A_a,
                            double *A_sc_l, int32_t *status)
{
    if (!c)
        return BQ_ERR_BAD_ARG;
    if (!x_sc || !l_sc || !mu || !cov || ns < 0 || nsc < ns || nsc < 1 || M < 0 ||
        (M && (!x_a || !A_a || !A_sc_l || !status)))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    const double wv[1] = {w};
    BQCHK(check_w(c, 1, h, wv, 0.0));
    if (M == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    EsmLayout L;
    L.ns = (int)ns;
    L.nsc = (int)nsc;
    L.npad = (int)roundup(nsc + 1, 64);
    L.ntot = L.npad + 64;
    const long lda = pick_ld(L.ntot);
    // per candidate: the bordered matrix, the panel scratch of the one-launch sweep, the
    // diagonal factor's record, failure flag and outputs
    const size_t per = sizeof(double) * ((size_t)lda * L.ntot +
                                         sweep_route(c, L.ntot, L.ntot, 1).ws_doubles +
                                         BQ_DINV_STRIDE + 2) + sizeof(int);
    size_t freeb = 0, totalb = 0;
    HIPCHK(c, hipMemGetInfo(&freeb, &totalb));
    int64_t chunk = std::max<int64_t>(1, (int64_t)((freeb / 2) / per));
    chunk = std::min<int64_t>(std::min<int64_t>(chunk, M), 32768);

    const GaussParams g = make_params(1, h, wv, 0.0);
    // jitter amounts exactly as two successive improve_covariance_conditioning calls
    // produce them (bq.py:470-476): max(K_l) is the kernel scale on the diagonal
    const double eps = std::numeric_limits<double>::epsilon();
    std::vector<double> j1((size_t)M), j2((size_t)M);
    for (int64_t a = 0; a < M; ++a) {
        bool any = false;
        for (int64_t j = ns; j < nsc && !any; ++j)
            any = std::fabs(x_sc[j] - x_a[a]) < thresh;
        const double first = any ? std::max(eps, g.c) * 1e-4 : 0.0;
        j1[(size_t)a] = first;
        j2[(size_t)a] = std::max(eps, g.c + first) * 1e-4;
    }

    DevBuf xs, ls, xa, ik, ika, dj1, dj2, Ad, dinv, info, outd, panel;
    HIPCHK(c, xs.alloc(sizeof(double) * nsc));
    HIPCHK(c, ls.alloc(sizeof(double) * nsc));
    HIPCHK(c, xa.alloc(sizeof(double) * M));
    HIPCHK(c, ik.alloc(sizeof(double) * nsc));
    HIPCHK(c, ika.alloc(sizeof(double) * M));
    HIPCHK(c, dj1.alloc(sizeof(double) * M));
    HIPCHK(c, dj2.alloc(sizeof(double) * M));
    HIPCHK(c, Ad.alloc(sizeof(double) * (size_t)lda * L.ntot * (size_t)chunk));
    HIPCHK(c, dinv.alloc(sizeof(double) * BQ_DINV_STRIDE * (size_t)chunk));
    HIPCHK(c,
           panel.alloc(sizeof(double) * sweep_route(c, L.ntot, L.ntot, (int)chunk).ws_doubles));
    HIPCHK(c, info.alloc(sizeof(int) * (size_t)chunk));
    HIPCHK(c, outd.alloc(sizeof(double) * 2 * (size_t)chunk));
    HIPCHK(c, hipMemcpyAsync(xs.p, x_sc, sizeof(double) * nsc, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(ls.p, l_sc, sizeof(double) * nsc, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(xa.p, x_a, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dj1.p, j1.data(), sizeof(double) * M, hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(dj2.p, j2.data(), sizeof(double) * M, hipMemcpyHostToDevice,
                             c->stream));
    // int K(x, .) p(x) dx at the nsc shared points and at every candidate
    const Small S = small_from_colmajor(cov, 1);
    const Small WS = cov_plus_w2(S, wv, 1.0);
    BQCHK(dev_int_K(c, 1, xs.d(), (int)nsc, mu, WS, h * h, 0.0, ik.d(), nullptr, nullptr, nullptr));
    BQCHK(dev_int_K(c, 1, xa.d(), (int)M, mu, WS, h * h, 0.0, ika.d(), nullptr, nullptr, nullptr));

    std::vector<double> hout((size_t)chunk * 2);
    std::vector<int> hinfo((size_t)chunk);
    for (int64_t a0 = 0; a0 < M; a0 += chunk) {
        const int nb = (int)std::min(chunk, M - a0);
        HIPCHK(c, hipMemsetAsync(info.p, 0, sizeof(int) * nb, c->stream));
        {
            Bracket br(c, BQ_K_GRAM, 8.0 * L.ntot * (L.ntot + 1.0) / 2.0 * nb);
            dim3 grid((L.ntot + 127) / 128, (L.ntot + 63) / 64, nb);
            hipLaunchKernelGGL(assemble_esm_kernel, grid, dim3(256), 0, c->stream, xs.d(),
                               xa.d() + a0, ik.d(), ika.d() + a0, ls.d(), dj1.d() + a0,
                               dj2.d() + a0, thresh, g, Ad.d(), lda, lda * (long)L.ntot, L);
            HIPCHK(c, hipGetLastError());
        }
        const SweepRoute route = sweep_route(c, L.ntot, L.npad, nb, panel.bytes / sizeof(double));
        BQCHK(enqueue_potrf_partial(c, route, Ad.d(), lda, lda * (long)L.ntot, dinv.d(), info.i(),
                                    panel.d()));
        hipLaunchKernelGGL(esm_finalize_kernel, dim3((nb + 255) / 256), dim3(256), 0, c->stream,
                           Ad.d(), lda, lda * (long)L.ntot, L, nb, outd.d());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hout.data(), outd.p, sizeof(double) * 2 * nb,
                                 hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hinfo.data(), info.p, sizeof(int) * nb, hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < nb; ++k) {
            A_a[a0 + k] = hout[(size_t)2 * k];
            A_sc_l[a0 + k] = hout[(size_t)2 * k + 1];
            status[a0 + k] = hinfo[(size_t)k];
        }
    }
    return BQ_OK;
}

// ===========================================================================
// The acquisition loop as a bordered UPDATE of the resident factor.
//
// For a candidate x_a the reference factors the (nsc + 1)^2 matrix
//     [ K_sc + J_c   k_a       ]     K_sc = K_l(x_sc, x_sc), k_a = K_l(x_sc, x_a),
//     [ k_a^T        k0 + j_a  ]     J_c: jitter on the candidates closer to x_a than thresh
// from scratch and solves it against b = int K_l(x_sca, x) p(x) dx (bq.py:463-480,
// bq_c.pyx:455-470).  K_sc is gp_l's own Gram matrix, whose factor L is resident: with
// M = K_sc + J_c,
//     A_a    = (b_a - k_a^T M^-1 b_sc) / (k0 + j_a - k_a^T M^-1 k_a)
//     A_sc.l = l^T M^-1 b_sc - A_a l^T M^-1 k_a.
// Every term is a bilinear form u^T M^-1 v = (L_M^-1 u) . (L_M^-1 v) of k_a (M of them), b_sc
// and l -- sums of products, so the Schur complement in the denominator is the difference of
// sums of squares that the reference's last pivot is.  The jitter sits on candidate points,
// the LAST rows of x_sc: with the factor cut at a column p <= ns,
//     L = [ L11 0 ; L21 L22 ],   L_M = [ L11 0 ; L21 L22' ],   L22' L22'^T = L22 L22^T + J_c,
// so one forward sweep F = R L^-T over the M + 2 rows gives the leading p entries of every
// L_M^-1 u as they stand, and the trailing nt = nsc - p (< nc + 64) entries are
// L22'^-1 (L22 F[p:]) -- an nt x nt Cholesky per DISTINCT set of jittered candidates and two
// nt x nt triangular products per candidate, on the host.  The device does the O(n^2 M) part:
// the sweep, one GEMM of the leading parts against b and l, the squared norms.  No inverse
// of K_sc is formed and nothing is subtracted but the Schur complement itself.  (A first
// version corrected K_sc^-1 by Woodbury: with the jitter larger than K_sc's small
// eigenvalues it lost cond(K) -- 3e-10 against the CPU restatement's 7e-13 on the ill-conditioned case
// of test_acquisition_and_posterior_vs_extended_precision.)  status[a] = 1 where the Schur
// complement is not positive (bq.py:481-490's fallback).  Requires a noise-free gp_l (Kxoxo
// carries no s^2 term, bq.py:465): BQ_ERR_BAD_ARG else, and the caller uses bq_esm_batch.
// ===========================================================================
// largest host tail / number of distinct jittered sets bq_esm_border takes on itself
#define BQ_ESM_MAX_TAIL 320
#define BQ_ESM_MAX_GROUPS 64

extern "C" int bq_esm_border(bq_ctx *c, bq_fit *gp_l, int64_t ns, const double *x_a, int64_t M,
                             double thresh, const double *mu, const double *cov, double *A_a,
                             double *A_sc_l, int32_t *status)
{
    BQCHK(check_fit(c, gp_l));
    if (gp_l->d != 1)
        return fail(c, BQ_ERR_BAD_ARG, "esm_border: one-dimensional fits only");
    if (gp_l->s != 0.0)
        return fail(c, BQ_ERR_BAD_ARG, "esm_border: gp_l carries a noise term");
    const int64_t nsc = gp_l->n;
    if (!mu || !cov || ns < 0 || ns > nsc || M < 0 || (M && (!x_a || !A_a || !A_sc_l || !status)))
        return fail(c, BQ_ERR_BAD_ARG, "illegal value");
    if (M == 0)
        return BQ_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const int nc = (int)(nsc - ns), npad = gp_l->npad;
    const int p = (int)(ns / 64 * 64);   // the cut: a multiple of 64 at or below ns
    const int nt = (int)nsc - p;         // trailing block handled on the host
    const double h = gp_l->h, wv[1] = {gp_l->w[0]};
    GaussParams g = make_params(1, h, wv, 0.0);
    // The trailing block lives on the host: an nt^3 / 3 Cholesky per DISTINCT set of jittered
    // candidates and O(nt^2) per candidate, single-threaded.  With many candidates (nt grows
    // with n_candidate) or many distinct sets that tail would dominate: then all candidates go
    // through the batched refactorisation on the device instead (bq_esm_batch).
    std::vector<double> xsc((size_t)nsc);
    HIPCHK(c, hipMemcpyAsync(xsc.data(), gp_l->pts.p, sizeof(double) * nsc, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    {
        std::vector<std::vector<int>> sets;
        std::vector<int> cl;
        for (int64_t a = 0; a < M && sets.size() <= BQ_ESM_MAX_GROUPS; ++a) {
            cl.clear();
            for (int i = 0; i < nc; ++i)
                if (std::fabs(xsc[(size_t)(ns + i)] - x_a[a]) < thresh)
                    cl.push_back(i);
            if (std::find(sets.begin(), sets.end(), cl) == sets.end())
                sets.push_back(cl);
        }
        if (nt > BQ_ESM_MAX_TAIL || sets.size() > BQ_ESM_MAX_GROUPS) {
            std::vector<double> lsc((size_t)nsc);
            HIPCHK(c, hipMemcpyAsync(lsc.data(), gp_l->y.p, sizeof(double) * nsc,
                                     hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return bq_esm_batch(c, xsc.data(), lsc.data(), ns, nsc, x_a, M, h, wv[0], thresh, mu,
                                cov, A_a, A_sc_l, status);
        }
    }
    // rows: [b_sc; l_sc; padding to 64] then the M borders
    const int T = 64, rb = 0, rl = 1;
    const int mrows = (int)roundup(T + M, 64);
    // temporaries from the context's scratch buffer (kept between calls: marginalize /
    // choose_next call this once per hyper-parameter sample)
    Scratch sc(c);
    const size_t oF = sc.take((size_t)mrows * npad), oG = sc.take((size_t)mrows * T),
                 oxa = sc.take((size_t)M), oik = sc.take((size_t)nsc), oika = sc.take((size_t)M),
                 osq = sc.take((size_t)mrows);
    BQCHK(sc.commit());
    struct View {
        double *q;
        void *p;
        double *d() const { return q; }
    };
    auto view = [&](size_t off) { return View{sc.at(off), sc.at(off)}; };
    const View F = view(oF), G = view(oG), xa = view(oxa), ik = view(oik), ika = view(oika),
               sq = view(osq);
    const View &R = F; // the sweep runs in place
    HIPCHK(c, hipMemcpyAsync(xa.p, x_a, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(R.p, 0, sizeof(double) * (size_t)mrows * npad, c->stream));
    HIPCHK(c, hipMemsetAsync(G.p, 0, sizeof(double) * (size_t)mrows * T, c->stream));
    HIPCHK(c, hipMemsetAsync(sq.p, 0, sizeof(double) * (size_t)mrows, c->stream));
    const Small S = small_from_colmajor(cov, 1);
    const Small WS = cov_plus_w2(S, wv, 1.0);
    BQCHK(dev_int_K(c, 1, gp_l->pts.d(), (int)nsc, mu, WS, h * h, 0.0, ik.d(), nullptr, nullptr,
                    nullptr));
    BQCHK(dev_int_K(c, 1, xa.d(), (int)M, mu, WS, h * h, 0.0, ika.d(), nullptr, nullptr, nullptr));
    HIPCHK(c, hipMemcpy2DAsync(R.d() + rb, sizeof(double) * mrows, ik.p, sizeof(double),
                               sizeof(double), nsc, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(R.d() + rl, sizeof(double) * mrows, gp_l->y.p, sizeof(double),
                               sizeof(double), nsc, hipMemcpyDeviceToDevice, c->stream));
    // rows T .. T + M - 1: the borders k_a^T
    BQCHK(launch_gram_cross(c, 1, xa.d(), (int)M, gp_l->pts.d(), (int)nsc, g, R.d() + T, mrows));
    // F = R L^-T (the accurate 64-column sweep, see enqueue_forward_rows_blk); over the leading
    // p columns G = -F F_tail^T (mrows x T) and the squared norms
    BQCHK(fit_dw(c, gp_l));
    BQCHK(enqueue_forward_rows_blk(c, F.d(), mrows, mrows, gp_l->A.d(), gp_l->ldl, npad,
                                   gp_l->dw.d()));
    if (p > 0) {
        GemmJob fft;
        fft.C = G.d(), fft.ldc = mrows;
        fft.P = F.d(), fft.ldp = mrows;
        fft.Q = F.d(), fft.qsj = 1, fft.qsk = mrows;
        fft.m = mrows, fft.n = T, fft.k = p;
        BQCHK(launch_gemm(c, BQ_K_GEMM, fft));
        BQCHK(launch_rowdot(c, F.d(), (long)mrows, mrows, mrows, p, nullptr, 0.0, nullptr, sq.d()));
    }
    // (of G only columns rb and rl -- the products with the b and l rows -- are read)
    std::vector<double> hG((size_t)mrows * 2), hsq((size_t)mrows), hb((size_t)M),
        F2((size_t)mrows * nt), L22((size_t)nt * nt);
    HIPCHK(c, hipMemcpyAsync(hG.data(), G.p, sizeof(double) * hG.size(), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(hsq.data(), sq.p, sizeof(double) * mrows, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(hb.data(), ika.p, sizeof(double) * M, hipMemcpyDeviceToHost,
                             c->stream));
    // F2[r + mrows j] = F[r, p + j]; L22[i + nt j] = L[p + i, p + j]
    HIPCHK(c, hipMemcpyAsync(F2.data(), F.d() + (size_t)p * mrows, sizeof(double) * F2.size(),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(L22.data(), sizeof(double) * nt,
                               gp_l->A.d() + p + (size_t)p * gp_l->ldl, sizeof(double) * gp_l->ldl,
                               sizeof(double) * nt, nt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int j = 1; j < nt; ++j) // strict upper triangle of the factor block is not the factor's
        for (int i = 0; i < j; ++i)
            L22[(size_t)i + (size_t)nt * j] = 0.0;
    // leading-part dot of any row r with tail row t (the GEMM stored its negative)
    auto dot1 = [&](int r, int t) { return p > 0 ? -hG[(size_t)r + (size_t)mrows * t] : 0.0; };
    // the trailing part of L_M^-1 u for row r: L22'^-1 (L22 F2[r, :])
    auto trail = [&](const std::vector<double> &Lm, bool same, int r, std::vector<double> &out) {
        out.assign((size_t)nt, 0.0);
        if (same) { // L22' = L22: the sweep's own entries
            for (int i = 0; i < nt; ++i)
                out[(size_t)i] = F2[(size_t)r + (size_t)mrows * i];
            return;
        }
        for (int i = 0; i < nt; ++i) { // w = L22 F2_r
            double v = 0.0;
            for (int q = 0; q <= i; ++q)
                v += L22[(size_t)i + (size_t)nt * q] * F2[(size_t)r + (size_t)mrows * q];
            out[(size_t)i] = v;
        }
        for (int i = 0; i < nt; ++i) { // forward substitution with L22'
            double v = out[(size_t)i];
            for (int q = 0; q < i; ++q)
                v -= Lm[(size_t)i + (size_t)nt * q] * out[(size_t)q];
            out[(size_t)i] = v / Lm[(size_t)i + (size_t)nt * i];
        }
    };
    auto vdot = [&](const std::vector<double> &u, const std::vector<double> &v) {
        double sacc = 0.0;
        for (int i = 0; i < nt; ++i)
            sacc += u[(size_t)i] * v[(size_t)i];
        return sacc;
    };
    // trailing Schur complement S22 = L22 L22^T
    std::vector<double> S22((size_t)nt * nt, 0.0);
    for (int j = 0; j < nt; ++j)
        for (int i = j; i < nt; ++i) {
            double v = 0.0;
            for (int q = 0; q <= j; ++q)
                v += L22[(size_t)i + (size_t)nt * q] * L22[(size_t)j + (size_t)nt * q];
            S22[(size_t)i + (size_t)nt * j] = v;
        }
    struct Group {
        std::vector<int> close;
        std::vector<double> Lm, fb, fl;
        double lMb = 0.0;
        bool ok = true;
    };
    std::vector<Group> groups;
    const double eps = std::numeric_limits<double>::epsilon();
    const double j1v = std::max(eps, g.c) * 1e-4;
    std::vector<int> close;
    std::vector<double> fa;
    for (int64_t a = 0; a < M; ++a) {
        const int ra = T + (int)a;
        close.clear();
        for (int i = 0; i < nc; ++i)
            if (std::fabs(xsc[(size_t)(ns + i)] - x_a[a]) < thresh)
                close.push_back(i);
        // jitter exactly as two successive improve_covariance_conditioning calls produce
        // it (bq.py:470-476): max(K_l) is the kernel scale on the diagonal
        const double j1 = close.empty() ? 0.0 : j1v;
        const double j2 = std::max(eps, g.c + j1) * 1e-4;
        Group *gr = nullptr;
        for (auto &q : groups)
            if (q.close == close)
                gr = &q;
        if (!gr) {
            groups.emplace_back();
            gr = &groups.back();
            gr->close = close;
            // L22' = chol(S22 + J_c) (the factor block itself when nothing is jittered)
            gr->Lm = close.empty() ? L22 : S22;
            if (!close.empty()) {
                for (int i : close)
                    gr->Lm[(size_t)(ns - p + i) * (nt + 1)] += j1;
                for (int k = 0; k < nt && gr->ok; ++k) {
                    double d = gr->Lm[(size_t)k + (size_t)nt * k];
                    for (int q = 0; q < k; ++q)
                        d -= gr->Lm[(size_t)k + (size_t)nt * q] * gr->Lm[(size_t)k + (size_t)nt * q];
                    if (!(d > 0.0)) {
                        gr->ok = false;
                        break;
                    }
                    d = std::sqrt(d);
                    gr->Lm[(size_t)k + (size_t)nt * k] = d;
                    for (int i = k + 1; i < nt; ++i) {
                        double v = gr->Lm[(size_t)i + (size_t)nt * k];
                        for (int q = 0; q < k; ++q)
                            v -= gr->Lm[(size_t)i + (size_t)nt * q] * gr->Lm[(size_t)k + (size_t)nt * q];
                        gr->Lm[(size_t)i + (size_t)nt * k] = v / d;
                    }
                }
            }
            if (gr->ok) {
                trail(gr->Lm, gr->close.empty(), rb, gr->fb);
                trail(gr->Lm, gr->close.empty(), rl, gr->fl);
                gr->lMb = dot1(rl, rb) + vdot(gr->fl, gr->fb);
            }
        }
        bool ok = gr->ok;
        double schur = 0.0, kMb = 0.0, lMk = 0.0;
        if (ok) {
            trail(gr->Lm, gr->close.empty(), ra, fa);
            const double kMk = -hsq[(size_t)ra] + vdot(fa, fa); // rowdot: 0 - |leading part|^2
            kMb = dot1(ra, rb) + vdot(fa, gr->fb);
            lMk = dot1(ra, rl) + vdot(fa, gr->fl);
            schur = g.c + j2 - kMk;
            ok = schur > 0.0 && std::isfinite(schur);
        }
        if (!ok) {
            status[a] = 1;
            A_a[a] = 0.0;
            A_sc_l[a] = 0.0;
            continue;
        }
        status[a] = 0;
        A_a[a] = (hb[(size_t)a] - kMb) / schur;
        A_sc_l[a] = gr->lMb - A_a[a] * lMk;
    }
    return BQ_OK;
}
