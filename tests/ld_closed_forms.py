"""Long-double references, float64 yardsticks, cases and bars of the closed-form layer: the Gram
kernels (csrc/gram.h), the four Gaussian integrals (csrc/moments.h, moments.hip) and E[Z], V(Z).
A helper module: test_closed_form_contracts.py holds the device to it, and
test_closed_form_contracts_host.py holds this module to independent derivations, on the CPU.

References (``numpy.longdouble``).  None shares the device's algebra: every integral is ONE joint
Gaussian log-density through one long-double Cholesky factor and a forward substitution -- no
explicit inverse, no S (W + S)^-1 S.  With S the measure's covariance, W = diag(w^2):

    int_K[i]               = h^2         N(x_i | mu, S + W)
    int_K1_K2[i, j]        = h1^2 h2^2   N([x1_i; x2_j] | [mu; mu], [[S + W1, S], [S, S + W2]])
    int_int_K1_K2[i]       = h1^2 h2^2   N([x_i; 0] | [mu; 0], [[S + W2, S], [S, 2 S + W1]])
    int_int_K1_K2_K1[i, j] = h1^4 h2^2   N([x_i; x_j; 0] | [mu; mu; 0],
                                           [[S + W1, 0, S], [0, S + W1, -S], [S, -S, 2 S + W2]])

(int_int_K1_K2: K_1 joins the two integration variables and K_2 the first of them to x_i, the
reference's gauss_c convention, which the oracle and the device follow; the known answers of
tests/golden pin it.)  ``ldc_*`` are the same integrals in long double by the conditional forms,
the algebra of csrc/moments.hip with explicit inverses: an independent derivation.

Yardsticks.  ``f64_stable_*`` are the four integrals in plain float64 numpy by an algebra without
cancellation: the conditional forms, factored blockwise, with S - S (W1 + S)^-1 S taken as
W1 - W1 (W1 + S)^-1 W1.  They stand for what float64 can deliver; their error against long double
is the ``r`` of the bars below, never the device's own algebra.

Units.  An entry's error is |got - ref| / |ref| / (1 + |E_ij|), E_ij = log(ref_ij / max ref): the
exponent is a sum of squares of size |E|, so a relative error in the small covariance algebra moves
the entry by about |E| times itself.  The device gets MARGIN max(r, 4 eps) in these units.

Gram bar, per entry, in ulps of the long-double value rounded to float64 (spacing floored at the
subnormal spacing): 2 ((D + 5) |q_ij| + 3 D + 4), q_ij the exponent.  gauss_q costs 6 roundings
per term (subtract, square, times nh, and nh's own 2: w * w and the division) plus D - 1 sums, all
of one sign, so the exponent carries at most (D + 5) relative roundings and the exp multiplies them
by |q|; make_params' c costs 3 D + 1 (h * h, and per axis the product sqrt(2 pi) w, its sqrt(2 pi)
and the division); the exp costs 1 ulp (test_exp_gauss_accuracy_on_probe_library); the product
c exp costs 1; one more for rounding the reference; the factor 2 converts a relative rounding of
one eps to ulps."""
import functools

import numpy as np

from test_gp_pivchol import _ld_solve_spd
from test_gp_sample import _LD_PI, _ld_gram
from test_gp_sample_host import kernel_scale

LD = np.longdouble
EPS = np.finfo(np.float64).eps
TINY = np.finfo(np.float64).tiny
MARGIN = 100.0  # the project's margin over a measured r (test_gp_zdesign.py, test_gp_ivr.py)


def _pts(x):
    x = np.asarray(x, dtype=np.float64)
    return np.asfortranarray(x[None, :] if x.ndim == 1 else x)


# ---- long double ----------------------------------------------------------------------------
def ld_gram(x1, x2, h, w):
    """k(x1_i, x2_j) in long double (test_gp_sample._ld_gram); points d x n."""
    return _ld_gram(_pts(x1), _pts(x2), h, np.atleast_1d(w))


def ld_gram_q(x1, x2, w):
    """The exponent q_ij = -sum_k (x1_ki - x2_kj)^2 / (2 w_k^2) in long double."""
    x1, x2, w = _pts(x1), _pts(x2), np.atleast_1d(w)
    q = np.zeros((x1.shape[1], x2.shape[1]), dtype=LD)
    for k in range(x1.shape[0]):
        t = x1[k].astype(LD)[:, None] - x2[k].astype(LD)[None, :]
        q += t * t / (LD(2) * LD(w[k]) ** 2)
    return -q


def ld_chol(A):
    n = A.shape[0]
    A = A.astype(LD)
    Lf = np.zeros((n, n), dtype=LD)
    for j in range(n):
        Lf[j, j] = np.sqrt(A[j, j] - Lf[j, :j] @ Lf[j, :j])
        Lf[j + 1:, j] = (A[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return Lf


def ld_log_density(Z, C):
    """log N(Z[:, k] | 0, C) for every column: one Cholesky factor, one forward substitution."""
    m = C.shape[0]
    Lf = ld_chol(C)
    Y = np.array(Z, dtype=LD)
    maha = np.zeros(Y.shape[1], dtype=LD)
    for j in range(m):
        Y[j] = (Y[j] - Lf[j, :j] @ Y[:j]) / Lf[j, j]
        maha += Y[j] * Y[j]
    return -LD(m) / 2 * np.log(LD(2) * _LD_PI) - np.sum(np.log(np.diag(Lf))) - maha / 2


def _ldm(w, mu, cov):
    d = len(np.atleast_1d(w))
    return (np.diag(np.atleast_1d(w).astype(LD) ** 2), np.atleast_1d(mu).astype(LD)[:, None],
            np.atleast_2d(cov).astype(LD).reshape(d, d))


def _logs(*hs):
    return sum(LD(2) * np.log(LD(abs(h))) for h in hs)


def ld_int_K(x, h, w, mu, cov, log=False):
    W, m, S = _ldm(w, mu, cov)
    out = _logs(h) + ld_log_density(_pts(x).astype(LD) - m, S + W)
    return out if log else np.exp(out)


def ld_int_K1_K2(x1, x2, h1, w1, h2, w2, mu, cov, log=False):
    x1, x2 = _pts(x1), _pts(x2)
    n1, n2 = x1.shape[1], x2.shape[1]
    W1, m, S = _ldm(w1, mu, cov)
    W2 = _ldm(w2, mu, cov)[0]
    Z = np.vstack([np.tile(x1.astype(LD) - m, (1, n2)), np.repeat(x2.astype(LD) - m, n1, axis=1)])
    out = _logs(h1, h2) + ld_log_density(Z, np.block([[S + W1, S], [S, S + W2]]))
    out = out.reshape(n2, n1).T
    return out if log else np.exp(out)


def ld_int_int_K1_K2(x, h1, w1, h2, w2, mu, cov, log=False):
    x = _pts(x)
    W1, m, S = _ldm(w1, mu, cov)
    W2 = _ldm(w2, mu, cov)[0]
    Z = np.vstack([x.astype(LD) - m, np.zeros(x.shape, dtype=LD)])
    out = _logs(h1, h2) + ld_log_density(Z, np.block([[S + W2, S], [S, 2 * S + W1]]))
    return out if log else np.exp(out)


def ld_int_int_K1_K2_K1(x, h1, w1, h2, w2, mu, cov, log=False):
    x = _pts(x)
    d, n = x.shape
    W1, m, S = _ldm(w1, mu, cov)
    W2 = _ldm(w2, mu, cov)[0]
    z = x.astype(LD) - m
    O = np.zeros((d, d), dtype=LD)
    Z = np.vstack([np.tile(z, (1, n)), np.repeat(z, n, axis=1), np.zeros((d, n * n), dtype=LD)])
    C = np.block([[S + W1, O, S], [O, S + W1, -S], [S, -S, 2 * S + W2]])
    out = _logs(h1, h1, h2) + ld_log_density(Z, C)
    out = out.reshape(n, n).T
    return out if log else np.exp(out)


# ---- the conditional forms in long double: the algebra of csrc/moments.hip --------------------
def _ld_inv(A):
    return _ld_solve_spd(A.astype(LD), np.eye(A.shape[0], dtype=LD))


def _ldc_logn(Z, C):
    """log N(Z[:, k] | 0, C) through the explicit inverse and the determinant of the factor."""
    Ci = _ld_inv(C)
    maha = np.sum(Z * (Ci @ Z), axis=0)
    logdet = 2 * np.sum(np.log(np.diag(ld_chol(C))))
    return -(LD(C.shape[0]) * np.log(LD(2) * _LD_PI) + logdet + maha) / 2


def ldc_int_K(x, h, w, mu, cov):
    W, m, S = _ldm(w, mu, cov)
    return _logs(h) + _ldc_logn(_pts(x).astype(LD) - m, S + W)


def ldc_int_K1_K2(x1, x2, h1, w1, h2, w2, mu, cov):
    """N(x1 | mu, S + W1) N(x2 - mu - G (x1 - mu) | 0, W2 + S - G S), G = S (S + W1)^-1."""
    x1, x2 = _pts(x1), _pts(x2)
    W1, m, S = _ldm(w1, mu, cov)
    W2 = _ldm(w2, mu, cov)[0]
    G = S @ _ld_inv(S + W1)
    z1, z2 = x1.astype(LD) - m, x2.astype(LD) - m
    a = _ldc_logn(z1, S + W1)
    g = G @ z1
    Cc = W2 + S - G @ S
    out = np.empty((x1.shape[1], x2.shape[1]), dtype=LD)
    for j in range(x2.shape[1]):
        out[:, j] = a + _ldc_logn(z2[:, j:j + 1] - g, Cc)
    return _logs(h1, h2) + out


def ldc_int_int_K1_K2(x, h1, w1, h2, w2, mu, cov):
    """bq_int_int_K1_K2's algebra: N(0 | 0, W1 + 2 S) N(x | mu, W2 + S - S (W1 + 2 S)^-1 S)."""
    x = _pts(x)
    d = x.shape[0]
    W1, m, S = _ldm(w1, mu, cov)
    W2 = _ldm(w2, mu, cov)[0]
    n0 = _ldc_logn(np.zeros((d, 1), dtype=LD), W1 + 2 * S)[0]
    return _logs(h1, h2) + n0 + _ldc_logn(x.astype(LD) - m, W2 + S - S @ _ld_inv(W1 + 2 * S) @ S)


def ldc_int_int_K1_K2_K1(x, h1, w1, h2, w2, mu, cov):
    """dev_iikk's algebra: n_i n_j N(G (x_i - x_j) | 0, W2 + 2 S - 2 G S), n = N(x | mu, W1 + S)."""
    x = _pts(x)
    n = x.shape[1]
    W1, m, S = _ldm(w1, mu, cov)
    W2 = _ldm(w2, mu, cov)[0]
    G = S @ _ld_inv(S + W1)
    nv = _ldc_logn(x.astype(LD) - m, S + W1)
    b = G @ x.astype(LD)
    Cm = W2 + 2 * S - 2 * (G @ S)
    out = np.empty((n, n), dtype=LD)
    for j in range(n):
        out[:, j] = nv + nv[j] + _ldc_logn(b - b[:, j:j + 1], Cm)
    return _logs(h1, h1, h2) + out


# ---- float64 without cancellation -------------------------------------------------------------
def stable_cond(S, W):
    """S - S (W + S)^-1 S as W - W (W + S)^-1 W, symmetrised: no cancellation for W small against
    S (the result is about W), none for S small against W (the correction is small)."""
    from scipy.linalg import cho_factor, cho_solve
    T = W - W @ cho_solve(cho_factor(W + S, lower=True), W)
    return 0.5 * (T + T.T)


def _f64m(w, mu, cov):
    d = len(np.atleast_1d(w))
    return (np.diag(np.atleast_1d(w).astype(np.float64) ** 2),
            np.atleast_1d(mu).astype(np.float64)[:, None],
            np.atleast_2d(cov).astype(np.float64).reshape(d, d))


def _f64_logn(Z, C):
    from scipy.linalg import solve_triangular
    Lf = np.linalg.cholesky(C)
    Y = solve_triangular(Lf, Z, lower=True)
    return -0.5 * C.shape[0] * np.log(2.0 * np.pi) - np.sum(np.log(np.diag(Lf))) - \
        0.5 * np.sum(Y * Y, axis=0)


def f64_stable_int_K(x, h, w, mu, cov):
    W, m, S = _f64m(w, mu, cov)
    return h * h * np.exp(_f64_logn(_pts(x) - m, S + W))


def f64_stable_int_K1_K2(x1, x2, h1, w1, h2, w2, mu, cov):
    """The factor of [[S + W1, S], [S, S + W2]] by blocks: L11 = chol(S + W1), L21 = S L11^-T,
    L22 = chol(W2 + W1 - W1 (S + W1)^-1 W1)."""
    from scipy.linalg import solve_triangular
    x1, x2 = _pts(x1), _pts(x2)
    W1, m, S = _f64m(w1, mu, cov)
    W2 = _f64m(w2, mu, cov)[0]
    L11 = np.linalg.cholesky(S + W1)
    L21 = solve_triangular(L11, S, lower=True).T
    L22 = np.linalg.cholesky(W2 + stable_cond(S, W1))
    y1 = solve_triangular(L11, x1 - m, lower=True)                       # d x n1
    a = -0.5 * np.sum(y1 * y1, axis=0)
    t = solve_triangular(L22, x2 - m, lower=True)                        # d x n2
    u = solve_triangular(L22, L21 @ y1, lower=True)                      # d x n1
    maha2 = np.sum((t[:, None, :] - u[:, :, None]) ** 2, axis=0)         # n1 x n2
    logc = -x1.shape[0] * np.log(2.0 * np.pi) - np.sum(np.log(np.diag(L11))) - \
        np.sum(np.log(np.diag(L22)))
    return (h1 * h1) * (h2 * h2) * np.exp(logc + a[:, None] - 0.5 * maha2)


def f64_stable_int_int_K1_K2(x, h1, w1, h2, w2, mu, cov):
    """S - S (W1 + 2 S)^-1 S is of the size of S: nothing cancels, the device's form stays."""
    from scipy.linalg import cho_factor, cho_solve
    x = _pts(x)
    d = x.shape[0]
    W1, m, S = _f64m(w1, mu, cov)
    W2 = _f64m(w2, mu, cov)[0]
    n0 = _f64_logn(np.zeros((d, 1)), W1 + 2.0 * S)[0]
    Cm = W2 + S - S @ cho_solve(cho_factor(W1 + 2.0 * S, lower=True), S)
    return (h1 * h1) * (h2 * h2) * np.exp(n0 + _f64_logn(x - m, 0.5 * (Cm + Cm.T)))


def f64_stable_int_int_K1_K2_K1(x, h1, w1, h2, w2, mu, cov):
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    x = _pts(x)
    W1, m, S = _f64m(w1, mu, cov)
    W2 = _f64m(w2, mu, cov)[0]
    nv = _f64_logn(x - m, S + W1)
    b = S @ cho_solve(cho_factor(S + W1, lower=True), x)
    Cm = W2 + 2.0 * stable_cond(S, W1)
    Lc = np.linalg.cholesky(Cm)
    y = solve_triangular(Lc, b, lower=True)
    maha = np.sum((y[:, :, None] - y[:, None, :]) ** 2, axis=0)
    logc = -0.5 * x.shape[0] * np.log(2.0 * np.pi) - np.sum(np.log(np.diag(Lc)))
    return (h1 * h1) ** 2 * (h2 * h2) * np.exp(nv[:, None] + nv[None, :] + logc - 0.5 * maha)


# ---- E[Z], V(Z) ---------------------------------------------------------------------------------
def ld_alpha(x, y, h, w, s):
    x = _pts(x)
    A = ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(x.shape[1], dtype=LD)
    return _ld_solve_spd(A, np.asarray(y, dtype=LD))


def ld_Z_mean(x_sc, l_sc, p_l, mu, cov):
    """(E[Z], sum_i |alpha_i kappa_i|): alpha = (K_l + s_l^2 I)^-1 l_sc, kappa = int_K."""
    h, w, s = p_l
    al = ld_alpha(x_sc, l_sc, h, w, s)
    kap = ld_int_K(x_sc, h, w, mu, cov)
    return al @ kap, np.sum(np.abs(al * kap))


def ld_Z_var(x_s, tl_s, x_sc, l_sc, p_tl, p_l, mu, cov):
    """(t1, t2, t1 - t2) of V(Z) = alpha' I3 alpha - beta' K_tl^-1 beta, beta = I2 alpha.  tl_s,
    the log-likelihoods at x_s, do not enter V(Z): K_tl depends on x_s alone."""
    (h1, w1, s1), (h2, w2, s2) = p_tl, p_l
    x_s = _pts(x_s)
    al = ld_alpha(x_sc, l_sc, h2, w2, s2)
    t1 = al @ ld_int_int_K1_K2_K1(x_sc, h2, w2, h1, w1, mu, cov) @ al
    beta = ld_int_K1_K2(x_s, x_sc, h1, w1, h2, w2, mu, cov) @ al
    Ktl = ld_gram(x_s, x_s, h1, w1) + LD(s1) ** 2 * np.eye(x_s.shape[1], dtype=LD)
    t2 = beta @ _ld_solve_spd(Ktl, beta)
    return t1, t2, t1 - t2


def f64_gram(x1, x2, h, w):
    x1, x2, w = _pts(x1), _pts(x2), np.atleast_1d(w)
    q = np.zeros((x1.shape[1], x2.shape[1]))
    for k in range(x1.shape[0]):
        t = x1[k][:, None] - x2[k][None, :]
        q += (t * t) * (-0.5 / (w[k] * w[k]))
    return kernel_scale(h, w) * np.exp(q)


def f64_Z(x_s, x_sc, l_sc, p_tl, p_l, mu, cov):
    """(E[Z], t1, t2) in float64: numpy's Cholesky solves around the f64_stable_* integrals."""
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    (h1, w1, s1), (h2, w2, s2) = p_tl, p_l
    x_s, x_sc = _pts(x_s), _pts(x_sc)
    Kl = f64_gram(x_sc, x_sc, h2, w2) + s2 * s2 * np.eye(x_sc.shape[1])
    al = cho_solve(cho_factor(Kl, lower=True), np.asarray(l_sc, dtype=np.float64))
    zm = al @ f64_stable_int_K(x_sc, h2, w2, mu, cov)
    t1 = al @ f64_stable_int_int_K1_K2_K1(x_sc, h2, w2, h1, w1, mu, cov) @ al
    beta = f64_stable_int_K1_K2(x_s, x_sc, h1, w1, h2, w2, mu, cov) @ al
    Lt = np.linalg.cholesky(f64_gram(x_s, x_s, h1, w1) + s1 * s1 * np.eye(x_s.shape[1]))
    v = solve_triangular(Lt, beta, lower=True)
    return zm, t1, v @ v


# ---- units and bars ---------------------------------------------------------------------------
def entry_units(got, ref):
    """|got - ref| / |ref| / (1 + |E|) per entry, E = log(ref / max ref); ref long double."""
    ref = np.asarray(ref, dtype=LD)
    E = np.log(ref / np.max(ref))
    return (np.abs(np.asarray(got).astype(LD) - ref) / ref / (1 + np.abs(E))).astype(np.float64)


def integral_bar(r):
    return MARGIN * max(r, 4 * EPS)


def all_normal(ref):
    r64 = np.asarray(ref).astype(np.float64)
    return bool(np.all(np.isfinite(r64)) and np.all(np.abs(r64) >= TINY))


def gram_ulps(K, ref):
    """|K - ref| in ulps of ref rounded to float64, the spacing floored at the subnormal one
    (test_exp_gauss_accuracy_on_probe_library)."""
    r64 = np.asarray(ref).astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(r64), TINY * 2.0 ** -52))
    return (np.abs(np.asarray(K).astype(LD) - ref) / ulp).astype(np.float64)


def gram_bound(q, D):
    return 2.0 * ((D + 5) * np.abs(np.asarray(q).astype(np.float64)) + 3 * D + 4)


def check_gram(K, case, cross=False):
    """The Gram bars on a device (or restated) matrix; returns the largest error over its bar."""
    ref, q, D = case["ref"], case["q"], case["d"]
    assert np.isfinite(K).all() and (K >= 0).all(), "Gram entries finite and not negative"
    err = gram_ulps(K, ref)
    bound = gram_bound(q, D)
    if not cross:
        n = K.shape[0]
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(K, K.T), "Gram symmetry"
        diag = LD(kernel_scale(case["h"], case["w"])) + LD(case["s"]) ** 2
        dulp = np.abs(np.diag(K).astype(LD) - diag) / np.spacing(np.float64(diag))
        assert float(dulp.max()) <= 4.0, ("Gram diagonal", float(dulp.max()))
        err, bound = err[off], bound[off]
        if err.size == 0:
            return 0.0
    worst = float(np.max(err / bound))
    assert worst <= 1.0, ("Gram per-entry ulps over the bound", worst)
    return worst


def check_integral(got, case, name, symmetric=False):
    """The integrals' bar on a device (or restated) result; returns the largest error in units of
    the bar."""
    ref, r = case[name], case["r"][name]
    got = np.asarray(got)
    assert got.shape == ref.shape and np.isfinite(got).all()
    if symmetric:
        assert np.array_equal(got, got.T), name + " bit symmetry"
    worst = float(np.max(entry_units(got, ref))) / integral_bar(r)
    assert worst <= 1.0, (name + " per-entry error over the bar", worst, r)
    return worst


# ---- cases --------------------------------------------------------------------------------------
D_ALL = tuple(range(1, 9))
GRAM_SIZES = (1, 2, 63, 64, 65, 128, 129, 192)
CROSS_SIZES = ((1, 1), (63, 65), (64, 16), (65, 17), (130, 77))
GRAM_H, GRAM_S = 0.9, 0.1


def gram_w(d):
    """Anisotropic: a factor 30 between the first and the last axis."""
    return 0.05 * 30.0 ** (np.arange(d) / max(d - 1, 1))


def gram_points(d, n, seed=0):
    """A cluster (q down to about -40) and, every twelfth point, an outlier whose distance from
    the cluster puts q around -726 (the subnormal results), -400, -770 (flushed), -260 or -600 in
    turn: normal, subnormal and flushed entries."""
    rs = np.random.RandomState(7919 * d + 13 * n + seed)
    u = rs.standard_normal((d, n)) * (1.6 / np.sqrt(d))
    for k, i in enumerate(range(1, n, 12)):
        v = rs.standard_normal(d)
        target = (726.0, 400.0, 770.0, 260.0, 600.0)[k % 5] + rs.uniform(-10.0, 10.0)
        u[:, i] += np.sqrt(2.0 * target) * v / np.linalg.norm(v)
    return np.asfortranarray(gram_w(d)[:, None] * u + 0.3)


@functools.lru_cache(maxsize=None)
def gram_case(d, n):
    x, w = gram_points(d, n), gram_w(d)
    ref = ld_gram(x, x, GRAM_H, w) + LD(GRAM_S) ** 2 * np.eye(n, dtype=LD)
    return dict(d=d, n=n, x=x, h=GRAM_H, w=w, s=GRAM_S, ref=ref, q=ld_gram_q(x, x, w))


@functools.lru_cache(maxsize=None)
def cross_case(d, n1, n2):
    x1, x2, w = gram_points(d, n1, 1), gram_points(d, n2, 2), gram_w(d)
    return dict(d=d, x1=x1, x2=x2, h=GRAM_H, w=w, s=0.0, ref=ld_gram(x1, x2, GRAM_H, w),
                q=ld_gram_q(x1, x2, w))


def gram_conditions(case):
    """Asserted on the reference alone (n >= 63): at least 80 % of the off-diagonal entries are
    normal numbers, at least 1 % lie below 1e-100 of the diagonal, and -- from 63 x 62 entries
    on -- subnormal and flushed entries occur."""
    ref = case["ref"]
    if ref.shape[0] == ref.shape[1] and "n" in case:
        off = ~np.eye(ref.shape[0], dtype=bool)
        r64, rl = ref.astype(np.float64)[off], ref[off]
        k0 = ref[0, 0]
    else:
        r64, rl = ref.astype(np.float64).ravel(), ref.ravel()
        k0 = LD(kernel_scale(case["h"], case["w"]))
    normal = np.mean(r64 >= TINY)
    small = np.mean(rl < LD(1e-100) * k0)
    assert normal >= 0.8 and small >= 0.01, (normal, small)
    if r64.size >= 63 * 62:
        assert np.any((r64 > 0) & (r64 < TINY)) and np.any(r64 == 0.0)
        assert float(np.max(case["q"])) <= 0.0 and float(np.min(case["q"])) < -745.0
    return float(normal), float(small)


FAMILIES = ("mild", "corr", "rho9", "aniso", "wide4e4", "wide4e6")
WIDE = ("wide4e4", "wide4e6")
VEC_SIZES = (1, 255, 256, 257)
K1K2_SIZES = ((1, 1), (63, 3), (64, 4), (65, 5), (130, 41))


def family_dims(fam):
    return (1, 2, 3) if fam in WIDE else D_ALL


def iikk_sizes(d):
    return (1, 63, 64, 65, 257) if d in (1, 8) else (1, 63, 64, 65)


def _corr_measure(d, rho):
    """test_gp_zdesign._measure with the correlation rho (0.3 there): off-centre."""
    mu = np.array([0.25 * (-1) ** k for k in range(d)])
    return mu, np.asfortranarray(1.5 ** 2 * ((1.0 - rho) * np.eye(d) + rho * np.ones((d, d))))


@functools.lru_cache(maxsize=None)
def family_params(fam, d):
    """(h1, w1, h2, w2, mu, cov, draw): draw(rs, n) gives d x n points for the family."""
    rs = np.random.RandomState(d)
    if fam == "mild":
        if d == 1:   # test_device_integrals_1d
            return (0.2, np.array([1.3]), 15.0, np.array([2.0]), np.array([0.3]),
                    np.array([[10.0]]), lambda r, n: np.sort(r.uniform(-5, 5, n))[None, :])
        rs.uniform(-2, 2, (d, 70)), rs.uniform(-2, 2, (d, 41))   # test_device_integrals_nd's draws
        w1, w2 = rs.uniform(0.5, 1.5, d), rs.uniform(0.5, 1.5, d)
        A = rs.rand(d, d)
        cov = A.dot(A.T) + d * np.eye(d)
        mu = rs.uniform(-0.5, 0.5, d)
        return 0.7, w1, 1.2, w2, mu, cov, lambda r, n: r.uniform(-2, 2, (d, n))
    if fam in ("corr", "rho9"):
        mu, cov = _corr_measure(d, 0.3 if fam == "corr" else 0.9)
        w1, w2 = rs.uniform(0.5, 1.5, d), rs.uniform(0.5, 1.5, d)
        return 0.7, w1, 1.2, w2, mu, cov, lambda r, n: r.uniform(-2, 2, (d, n))
    if fam == "aniso":
        mu, cov = _corr_measure(d, 0.3)
        w1 = 0.1 * 30.0 ** (np.arange(d) / max(d - 1, 1))
        w2 = 1.3 * w1[::-1]
        return (0.7, w1, 1.2, w2, mu, cov,
                lambda r, n: 0.5 + 3.0 * w1[:, None] * r.uniform(-1, 1, (d, n)))
    # a measure wide against the length scales: cov / w1^2 = ratio (C2: n = 1024, w = 1.5 dx,
    # cov = 10 gives 4e4); the points are one off-centre cluster, so that no entry underflows
    ratio = {"wide4e4": 4e4, "wide4e6": 4e6}[fam]
    mu = np.full(d, 0.3)
    cov = 10.0 * (0.7 * np.eye(d) + 0.3 * np.ones((d, d))) if d > 1 else np.array([[10.0]])
    w1 = np.sqrt(10.0 / ratio) * np.array([1.0, 1.2, 0.9])[:d]
    centre = np.array([2.0, -1.0, 1.5])[:d]
    a = 25.0 / np.sqrt(d)
    return (0.2, w1, 15.0, 1.5 * w1, mu, cov,
            lambda r, n: centre[:, None] + w1[:, None] * r.uniform(-a, a, (d, n)))


def family_points(fam, d, n, seed):
    draw = family_params(fam, d)[6]
    return np.asfortranarray(draw(np.random.RandomState(100003 * seed + 101 * d + n), n))


_F64 = dict(int_K=f64_stable_int_K, int_K1_K2=f64_stable_int_K1_K2,
            int_int_K1_K2=f64_stable_int_int_K1_K2, int_int_K1_K2_K1=f64_stable_int_int_K1_K2_K1)
_LDF = dict(int_K=ld_int_K, int_K1_K2=ld_int_K1_K2, int_int_K1_K2=ld_int_int_K1_K2,
            int_int_K1_K2_K1=ld_int_int_K1_K2_K1)


@functools.lru_cache(maxsize=None)
def integral_case(fam, d, name, size):
    """The inputs, the long-double reference and the measured r of one entry point at one size:
    {"args": what the entry point takes, name: reference, "r": {name: r}}."""
    h1, w1, h2, w2, mu, cov, _ = family_params(fam, d)
    if name == "int_K":
        args = (family_points(fam, d, size, 1), h1, w1, mu, cov)
    elif name == "int_K1_K2":
        args = (family_points(fam, d, size[0], 2), family_points(fam, d, size[1], 3), h1, w1, h2,
                w2, mu, cov)
    else:
        args = (family_points(fam, d, size, 4), h1, w1, h2, w2, mu, cov)
    ref = _LDF[name](*args)
    r = float(np.max(entry_units(_F64[name](*args), ref)))
    return {"args": args, name: ref, "r": {name: r}}


def integral_sizes(name, d):
    return {"int_K": VEC_SIZES, "int_int_K1_K2": VEC_SIZES, "int_K1_K2": K1K2_SIZES,
            "int_int_K1_K2_K1": iikk_sizes(d)}[name]


# (d, ns, nc, s_l, wide): gp_tl's noise is 0.1 throughout
MOMENT_D = (1, 2, 3, 8)
MOMENT_SIZES = ((65, 5), (130, 17), (200, 70))
MOMENT_CASES = [(d, ns, nc, s_l, False) for d in MOMENT_D for (ns, nc) in MOMENT_SIZES
                for s_l in (1e-3, 0.0)] + [(1, 130, 17, 1e-3, True), (2, 130, 17, 1e-3, True)]
S_TL = 0.1


def _norm_logpdf(x):
    return -0.5 * np.sum(x * x, axis=0) - 0.5 * x.shape[0] * np.log(2.0 * np.pi)


@functools.lru_cache(maxsize=None)
def moment_case(d, ns, nc, s_l, wide):
    """The inputs of one E[Z] / V(Z) case, the long-double answers and the measured r."""
    rs = np.random.RandomState(1000 * d + ns)
    if d == 1:   # test_device_moments_vs_oracle's observations and length scales
        dx = 10.0 / (ns - 1)
        xs = (np.linspace(-5, 5, ns) + rs.uniform(-dx / 4, dx / 4, ns))[None, :]
        # (candidates between neighbouring observations, no closer than dx / 8 to either: K_l
        # stays factorable without noise)
        gaps = np.sort(rs.permutation(ns - 1)[:nc])
        xc = (0.5 * (xs[0, gaps] + xs[0, gaps + 1]) + rs.uniform(-dx / 16, dx / 16, nc))[None, :]
        w_tl = w_l = np.array([1.5 * dx])
        mu, cov = np.array([0.3]), np.array([[10.0]])
    else:
        xs, xc = rs.uniform(-2, 2, (d, ns)), rs.uniform(-2.5, 2.5, (d, nc))
        # (length scales that leave K_l, 270 points in the box, factorable without noise)
        w_tl = rs.uniform(0.8, 1.6, d) * {2: 0.3, 3: 0.8}.get(d, 1.0)
        w_l = 0.9 * w_tl
        mu, cov = _corr_measure(d, 0.3)
    if wide:   # cov / w_l^2 about 4e4, C2's regime
        cov = cov * (4e4 * float(np.mean(w_l ** 2)) / float(np.mean(np.diag(cov))))
    xsc = np.asfortranarray(np.hstack([xs, xc]))
    xs = np.asfortranarray(xs)
    ls, lsc = np.exp(_norm_logpdf(xs)), np.exp(_norm_logpdf(xsc))
    p_tl, p_l = (15.0, w_tl, S_TL), (0.2, w_l, s_l)
    zm, zabs = ld_Z_mean(xsc, lsc, p_l, mu, cov)
    t1, t2, zv = ld_Z_var(xs, np.log(ls), xsc, lsc, p_tl, p_l, mu, cov)
    zm64, t164, t264 = f64_Z(xs, xsc, lsc, p_tl, p_l, mu, cov)
    return dict(xs=xs, ls=ls, xsc=xsc, lsc=lsc, p_tl=p_tl, p_l=p_l, mu=mu,
                cov=np.asfortranarray(cov), zm=zm, zabs=zabs, t1=t1, t2=t2, zv=zv,
                r_mean=float(abs(LD(zm64) - zm) / zabs),
                r_Z=float(abs((LD(t164) - LD(t264)) - zv) / abs(t1)),
                ratio=float(t2 / t1))


def check_Z_mean(got, case):
    worst = float(abs(LD(got) - case["zm"]) / case["zabs"]) / integral_bar(case["r_mean"])
    assert worst <= 1.0, ("Z_mean over the bar", worst, case["r_mean"])
    return worst


def check_Z_var(got, case):
    worst = float(abs(LD(got) - case["zv"]) / abs(case["t1"])) / integral_bar(case["r_Z"])
    assert worst <= 1.0, ("Z_var over the bar", worst, case["r_Z"], case["ratio"])
    return worst
