"""CPU tests of square-root-warped Bayesian quadrature (WSABI-L): the contracts of bq_gp_sqintegral
and bq_gp_sqdesign restated in numpy -- the closed forms ``W_closed``, ``Q_closed`` and
``kappa_closed`` in the precision of their arguments, ``numpy_sqintegral`` and ``numpy_squ0``, with
test_gp_zdesign_host.numpy_zdesign for the recurrence --, the restatement checked against
Gauss-Hermite quadrature, its properties, and the host plumbing (engine.Fit.sq_integral* as
gp.GP.sq_integral*, wsabi.SqrtBQ and BQ.sqrt_bq use them) over the oracle-backed engine double.
test_gp_sqwarp.py holds the device to the same contracts."""
import pickle

import numpy as np
import pytest
from numpy.polynomial.hermite_e import hermegauss

from test_gp_pivchol_host import OPTIONS
from test_gp_sample_host import kernel_scale
from test_gp_zdesign_host import ZdEngineDouble, ZdFitDouble, numpy_zdesign
from test_predict_grad_host import numpy_predict_grad

EPS = np.finfo(np.float64).eps


# ---- the closed forms, in the precision of their arguments ----

def _chol(Am):
    n = Am.shape[0]
    Lf = np.zeros((n, n), dtype=Am.dtype)
    for j in range(n):
        Lf[j, j] = np.sqrt(Am[j, j] - Lf[j, :j] @ Lf[j, :j])
        Lf[j + 1:, j] = (Am[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return Lf


def _small_solve(Cm, B):
    """Cm^-1 B for a small SPD Cm by its Cholesky factor."""
    Lf = _chol(Cm)
    n = Cm.shape[0]
    Y = np.array(B, dtype=Cm.dtype)
    for j in range(n):
        Y[j] = (Y[j] - Lf[j, :j] @ Y[:j]) / Lf[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - Lf[j + 1:, j] @ Y[j + 1:]) / Lf[j, j]
    return Y


def _log_pdf0(z, Cm):
    """log N(z | 0, Cm) for z of shape (d, ...)."""
    dt = Cm.dtype.type
    d = Cm.shape[0]
    Lf = _chol(Cm)
    y = np.array(z, dtype=Cm.dtype)
    for j in range(d):
        y[j] = (y[j] - np.tensordot(Lf[j, :j], y[:j], axes=(0, 0))) / Lf[j, j]
    two_pi = dt(8) * np.arctan(dt(1))
    return -dt(d) / 2 * np.log(two_pi) - np.sum(np.log(np.diag(Lf))) - np.sum(y * y, axis=0) / 2


def _args(h, w, mu, cov, *pts):
    dt = np.result_type(*[np.asarray(p).dtype for p in pts], np.float64)
    w = np.atleast_1d(np.asarray(w, dtype=dt))
    return (dt.type(h), np.diag(w * w), np.atleast_1d(np.asarray(mu, dtype=dt)),
            np.atleast_2d(np.asarray(cov, dtype=dt))) + tuple(np.asarray(p, dtype=dt) for p in pts)


def gram_closed(a, b, h, w):
    """k(a_i, b_j) = h^2 N(a_i | b_j, diag(w^2)) for points (d, P) and (d, Q)."""
    h, Lam, _, _, a, b = _args(h, w, 0.0, 1.0, a, b)
    return h * h * np.exp(_log_pdf0(a[:, :, None] - b[:, None, :], Lam))


def kappa_closed(x, h, w, mu, cov):
    """kappa_i = h^2 N(x_i | mu, Lambda + Sigma)."""
    h, Lam, mu, cov, x = _args(h, w, mu, cov, x)
    return h * h * np.exp(_log_pdf0(x - mu[:, None], Lam + cov))


def W_closed(p, q, h, w, mu, cov):
    """W(p_i, q_j) = int k(p_i, t) k(t, q_j) N(t | mu, Sigma) dt
    = h^4 N(p - q | 0, 2 Lambda) N((p + q) / 2 | mu, Lambda / 2 + Sigma)."""
    h, Lam, mu, cov, p, q = _args(h, w, mu, cov, p, q)
    dif = p[:, :, None] - q[:, None, :]
    mid = (p[:, :, None] + q[:, None, :]) / 2 - mu[:, None, None]
    return h ** 4 * np.exp(_log_pdf0(dif, 2 * Lam) + _log_pdf0(mid, Lam / 2 + cov))


def Q_closed(x, h, w, mu, cov):
    """Q_ij = int int k(x_i, t) k(t, t') k(t', x_j) N(t) N(t') = h^2 kappa_i kappa_j
    N(S Lambda^-1 (x_i - x_j) | 0, Lambda + 2 S), S = (Lambda^-1 + Sigma^-1)^-1."""
    h, Lam, mu, cov, x = _args(h, w, mu, cov, x)
    G = _small_solve(Lam + cov, cov).T   # Sigma (Lambda + Sigma)^-1 = S Lambda^-1
    S = G @ Lam
    kap = kappa_closed(x, h, np.sqrt(np.diag(Lam)), mu, cov)
    z = np.tensordot(G, x[:, :, None] - x[:, None, :], axes=(1, 0))
    return h * h * kap[:, None] * kap[None, :] * np.exp(_log_pdf0(z, Lam + 2 * (S + S.T) / 2))


def numpy_sqintegral(Wxx, Qxx, Kxx, y):
    """(sq, var, r, alpha, b_w, qq): the contract of bq_gp_sqintegral in float64 from W(X, X), Q,
    Kxx = K + s^2 I and the warped targets: alpha = Kxx^-1 y, r = W alpha, sq = alpha . r,
    b_w = L^-1 r, qq = alpha^T Q alpha, var = qq - b_w . b_w (not clamped)."""
    L = np.linalg.cholesky(Kxx)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    r = Wxx @ alpha
    b = np.linalg.solve(L, r)
    qq = alpha @ Qxx @ alpha
    return alpha @ r, qq - b @ b, r, alpha, b, qq


def numpy_squ0(Wcx, Kcx, Kxx, alpha, r):
    """u_a = Cov(Z, g(c_a) | data) = sum_j W(c_a, x_j) alpha_j - k(c_a, X) Kxx^-1 r."""
    return Wcx @ alpha - Kcx @ np.linalg.solve(Kxx, r)


# ---- the restatement against Gauss-Hermite quadrature ----

def _problem(d, n=12, seed=0):
    """A positive integrand at n points, its warped targets, a kernel, and a correlated
    off-centre measure."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-2.5, 2.5, size=(d, n))
    l = np.exp(-0.5 * np.sum((x - 0.4) ** 2, axis=0) / 0.8 ** 2) + 0.05
    a0 = 0.8 * l.min()
    mu = np.array([0.3, -0.2])[:d]
    cov = 1.2 ** 2 * (0.7 * np.eye(d) + 0.3 * np.ones((d, d)))
    c = rs.uniform(-2.5, 2.5, size=(d, 4))
    return x, np.sqrt(2 * (l - a0)), 1.1, np.full(d, 0.9), 0.05, mu, cov, c


def _restated(x, y, h, w, s, mu, cov, c):
    Kxx = gram_closed(x, x, h, w) + s * s * np.eye(x.shape[1])
    sq, var, r, alpha, b, qq = numpy_sqintegral(W_closed(x, x, h, w, mu, cov),
                                                Q_closed(x, h, w, mu, cov), Kxx, y)
    u = numpy_squ0(W_closed(c, x, h, w, mu, cov), gram_closed(c, x, h, w), Kxx, alpha, r)
    return sq, var, u


def _quadrature(nn, x, y, h, w, s, mu, cov, c):
    """(sq, var, u, their scales): int m^2 pi, int int m Sigma m pi pi and int m Sigma(., c) pi on
    the tensor Gauss-Hermite grid of nn nodes per axis mapped through the Cholesky factor of the
    measure's covariance; the scales are the same sums over absolute values."""
    d = x.shape[0]
    t, wt = hermegauss(nn)
    T = np.stack(np.meshgrid(*([t] * d), indexing="ij")).reshape(d, -1)
    pw = np.prod(np.stack(np.meshgrid(*([wt] * d), indexing="ij")).reshape(d, -1), axis=0)
    pw = pw / (2 * np.pi) ** (d / 2)
    g = mu[:, None] + np.linalg.cholesky(cov) @ T
    Kxx = gram_closed(x, x, h, w) + s * s * np.eye(x.shape[1])
    kg = gram_closed(g, x, h, w)
    m = kg @ np.linalg.solve(Kxx, y)
    v = m * pw
    kv = kg.T @ v
    vKv = sum(v[i:i + 600] @ (gram_closed(g[:, i:i + 600], g, h, w) @ v)
              for i in range(0, g.shape[1], 600))
    red = kv @ np.linalg.solve(Kxx, kv)
    Kcx = gram_closed(c, x, h, w)
    u = gram_closed(c, g, h, w) @ v - Kcx @ np.linalg.solve(Kxx, kv)
    scales = ((m * m) @ pw, vKv + red, np.abs(gram_closed(c, g, h, w)) @ np.abs(v))
    return (m * m) @ pw, vKv - red, u, scales


@pytest.mark.parametrize("d,nn,finer", [(1, 120, 160), (2, 60, 80)])
def test_closed_forms_agree_with_gauss_hermite_quadrature(d, nn, finer):
    """sq, the variance and u at four candidates against tensor Gauss-Hermite quadrature.  The
    tolerance is the quadrature's own: ten times the change from nn to `finer` nodes per axis, plus
    the rounding that both sides share in float64 -- every term passes through Kxx^-1, so
    eps cond(Kxx) times the size of the terms, with a factor 10 as well."""
    pr = _problem(d)
    x, y, h, w, s = pr[:5]
    sq, var, u = _restated(*pr)
    a, b = _quadrature(nn, *pr), _quadrature(finer, *pr)
    cond = np.linalg.cond(gram_closed(x, x, h, w) + s * s * np.eye(x.shape[1]))
    for k, (name, got) in enumerate((("sq", sq), ("var", var), ("u", u))):
        qa, qb, scale = a[k], b[k], a[3][k]
        conv = float(np.max(np.abs(qa - qb)))
        tol = 10 * conv + 10 * EPS * cond * float(np.max(scale))
        err = float(np.max(np.abs(got - qa)))
        print("d=%d %s: error %.3g, quadrature's change %.3g, rounding share %.3g"
              % (d, name, err, conv, tol - 10 * conv))
        assert err <= tol
    assert var > 0 and sq > 0


# ---- properties of the restatement ----

def _design_case(nu, seed=1, A=18, n=10):
    rs = np.random.RandomState(seed)
    x, c = rs.uniform(-3, 3, size=(1, n)), rs.uniform(-3, 3, size=(1, A))
    l = np.exp(-0.5 * (x[0] - 0.4) ** 2 / 0.7 ** 2) + 0.02
    a0 = 0.8 * l.min()
    y = np.sqrt(2 * (l - a0))
    h, w, s, mu, cov = 1.0, [0.8], 0.3, [0.4], [[1.3 ** 2]]
    Kxx = gram_closed(x, x, h, w) + s * s * np.eye(n)
    sq, var, r, alpha, b, qq = numpy_sqintegral(W_closed(x, x, h, w, mu, cov),
                                                Q_closed(x, h, w, mu, cov), Kxx, y)
    Kcx = gram_closed(c, x, h, w)
    u0 = numpy_squ0(W_closed(c, x, h, w, mu, cov), Kcx, Kxx, alpha, r)
    Sig = gram_closed(c, c, h, w) - Kcx @ np.linalg.solve(Kxx, Kcx.T)
    return dict(x=x, c=c, y=y, a0=a0, h=h, w=w, s=s, mu=mu, cov=cov, Kxx=Kxx, alpha=alpha, Sig=Sig,
                u0=u0, var=var, qq=qq, Kcx=Kcx)


@pytest.mark.parametrize("nu", [0.0, 0.09])
def test_restatement_gains_telescope_and_prefixes(nu):
    """The variance of the warped integral drops by exactly the gain at every step -- recomputed
    from the definition with the chosen candidates observed and the mean held --, and the runs
    are prefixes of one another."""
    p = _design_case(nu)
    full = numpy_zdesign(p["Sig"], p["u0"], p["var"], p["qq"], 1.0, 8, nu)
    assert full[6] == 8 and np.all(full[1] > 0)
    for j in range(1, 9):
        piv, gain, z0, ru, rc, s0, rank = numpy_zdesign(p["Sig"], p["u0"], p["var"], p["qq"], 1.0,
                                                        j, nu)
        assert rank == j and np.array_equal(piv, full[0][:j]) and np.array_equal(gain, full[1][:j])
        assert np.array_equal(s0, full[5])
        S = p["Sig"][np.ix_(piv, piv)] + nu * np.eye(j)
        after = p["var"] - p["u0"][piv] @ np.linalg.solve(S, p["u0"][piv])
        assert abs(after - (p["var"] - gain.sum())) <= 1e-13 * p["qq"]
    assert p["var"] - full[1].sum() > 0


def test_restatement_gains_are_the_variance_after_appending_the_picks_at_their_mean():
    """var0 - sum gain equals bq_gp_sqintegral's variance after the picks have been appended with
    noise s^2 and targets equal to the current latent mean there: such observations leave m
    unchanged, and with it the functional."""
    p = _design_case(0.09)
    s, h, w, mu, cov = p["s"], p["h"], p["w"], p["mu"], p["cov"]
    piv, gain = numpy_zdesign(p["Sig"], p["u0"], p["var"], p["qq"], 1.0, 6, s * s)[:2]
    x2 = np.concatenate([p["x"], p["c"][:, piv]], axis=1)
    y2 = np.concatenate([p["y"], p["Kcx"][piv] @ p["alpha"]])
    K2 = gram_closed(x2, x2, h, w) + s * s * np.eye(x2.shape[1])
    sq2, var2, _, alpha2, _, _ = numpy_sqintegral(W_closed(x2, x2, h, w, mu, cov),
                                                  Q_closed(x2, h, w, mu, cov), K2, y2)
    grid = np.linspace(-4, 4, 41)[None, :]
    m1 = gram_closed(grid, p["x"], h, w) @ p["alpha"]
    m2 = gram_closed(grid, x2, h, w) @ alpha2
    assert np.max(np.abs(m1 - m2)) <= 1e-11 * np.max(np.abs(m1))  # the mean is held
    print("variance after append %.17g, telescoped %.17g" % (var2, p["var"] - gain.sum()))
    assert abs(var2 - (p["var"] - gain.sum())) <= 1e-11 * p["qq"]


def test_restatement_l_mean_is_never_below_alpha0():
    p = _design_case(0.0)
    grid = np.linspace(-6, 6, 481)[None, :]
    m = gram_closed(grid, p["x"], p["h"], p["w"]) @ p["alpha"]
    assert np.all(p["a0"] + 0.5 * m * m >= p["a0"]) and p["a0"] > 0
    # ... also where the warped GP's own mean changes sign: the same points with targets that do
    y = p["y"] - p["y"].mean()
    m = gram_closed(grid, p["x"], p["h"], p["w"]) @ np.linalg.solve(p["Kxx"], y)
    assert np.any(m < 0) and np.all(p["a0"] + 0.5 * m * m >= p["a0"])


# ---- the engine double ----

class SqFitDouble(ZdFitDouble):
    """ZdFitDouble with ``sq_integral`` and ``sq_integral_design`` over the closed forms above,
    ``predict_grad`` (for the acquisition's gradient), ``append`` and ``remove``."""

    def _x2(self):
        return np.atleast_2d(self.x)

    def _sq(self, mu, cov):
        x = self._x2()
        return numpy_sqintegral(W_closed(x, x, self.h, self.w, mu, cov),
                                Q_closed(x, self.h, self.w, mu, cov), np.asarray(self.K()), self.y)

    def sq_integral(self, mu, cov, want_r=False):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        mu, cov = self._measure(mu, cov)
        self.calls.append(("sq_integral", mu.copy(), cov.copy(), want_r, self.h))
        sq, var, r = self._sq(mu, cov)[:3]
        res = (float(sq), float(var))
        return res + (r,) if want_r else res

    def sq_integral_design(self, xc, q, mu, cov, nugget=0.0, tol=0.0, want_scores=False):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        xc = self._pts(xc)
        mu, cov = self._measure(mu, cov)
        self.calls.append(("sqdesign", xc.shape[1], q, nugget, tol, self.h, mu.copy(), cov.copy()))
        sq, var, r, alpha, b, qq = self._sq(mu, cov)
        x = self._x2()
        u0 = numpy_squ0(W_closed(xc, x, self.h, self.w, mu, cov),
                        gram_closed(xc, x, self.h, self.w), np.asarray(self.K()), alpha, r)
        _, _, Sig = self.predict(xc if self.d > 1 else xc[0], want_cov=True)
        piv, gain, zvar0, ru, rc, s0, rk = numpy_zdesign(
            np.asarray(Sig), u0, float(var), float(qq), kernel_scale(self.h, self.w), q, nugget, tol)
        res = (piv[:rk], gain[:rk], float(zvar0), ru, rc)
        return res + (s0,) if want_scores else res

    def predict_grad(self, xo, want_var=True):
        xo = np.asarray(xo, dtype=np.float64)
        xo = xo[None, :] if xo.ndim == 1 else xo
        return numpy_predict_grad(self.o, self.x, self.y, self.h, self.w, self.s, xo, want_var)

    def _regrow(self, x, y):
        self.x, self.y = x, y
        self.n = self.y.shape[0]
        self._L, self._alpha, self.logml = self.o.gp_fit(self.x, self.y, self.h, self.w, self.s)

    def append(self, x_new, y_new):
        self.calls.append(("append", np.size(y_new)))
        self._regrow(np.concatenate([np.ravel(self.x), np.ravel(x_new)]),
                     np.concatenate([self.y, np.ravel(y_new)]))

    def remove(self, idx):
        self.calls.append(("remove", np.size(idx)))
        self._regrow(np.delete(np.ravel(self.x), idx), np.delete(self.y, idx))


class SqEngineDouble(ZdEngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return SqFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def pkg(oracle):
    import bayesian_quadrature_amd as pkg
    from bayesian_quadrature_amd import engine as eng_mod
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(SqEngineDouble(oracle), 0)
    yield pkg
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _samples(n=13):
    x = np.linspace(-3, 3, n)
    return x, np.exp(-0.5 * (x - 0.4) ** 2 / 0.3 ** 2)


# ---- the demonstration ----

def test_warped_mean_stays_positive_where_the_vanilla_mean_does_not(pkg):
    """l = exp(-(x - 0.4)^2 / (2 0.3^2)) at 13 points on [-3, 3], prior N(0, 1), h = 1, w = 0.6,
    s = 1e-3.  The vanilla GP on l has a posterior mean that goes down to -0.067 between the
    samples; the warped l_mean is >= alpha0 >= 0 everywhere.  Both integrals are within two of
    their own standard deviations of the truth 0.267013 (errors -2.0e-4 vanilla and -1.8e-4
    warped at these fixed hyper-parameters: a tie, and not asserted)."""
    from bayesian_quadrature_amd.wsabi import SqrtBQ
    x, l = _samples()
    truth = 0.3 / np.sqrt(0.3 ** 2 + 1.0) * np.exp(-0.5 * 0.4 ** 2 / (0.3 ** 2 + 1.0))
    assert abs(truth - 0.267013) < 1e-6
    vanilla = pkg.GP(pkg.GaussianKernel(1.0, 0.6), x, l, s=1e-3)
    sb = SqrtBQ(x, l, pkg.GaussianKernel(1.0, 0.6), 1e-3, 0.0, 1.0)
    grid = np.linspace(-3.0, 3.0, 1201)
    vm, wm = vanilla.mean(grid), sb.l_mean(grid)
    zv, vv = vanilla.integral(0.0, 1.0)
    zw, vw = sb.integral()
    print("vanilla: min mean %.4f, Z %.6f (error %.2g, sd %.2g); warped: min l_mean %.4g, alpha0 "
          "%.4g, Z %.6f (error %.2g, sd %.2g)" % (vm.min(), zv, zv - truth, np.sqrt(vv), wm.min(),
                                                  sb.alpha0, zw, zw - truth, np.sqrt(vw)))
    assert vm.min() < 0
    assert sb.alpha0 >= 0 and np.all(wm >= sb.alpha0)
    assert vv > 0 and abs(zv - truth) <= 2 * np.sqrt(vv)
    assert vw > 0 and abs(zw - truth) <= 2 * np.sqrt(vw)


# ---- the plumbing ----

def test_signatures_are_declared():
    from bayesian_quadrature_amd import _lib
    assert _lib.SIGNATURES["bq_gp_sqintegral"] == _lib.SIGNATURES["bq_gp_integral"]
    assert _lib.SIGNATURES["bq_gp_sqdesign"] == _lib.SIGNATURES["bq_gp_zdesign"]


def test_fit_double_stands_in_for_the_engine_s_fit():
    import inspect
    from bayesian_quadrature_amd import engine
    for name in ("sq_integral", "sq_integral_design"):
        assert (inspect.signature(getattr(engine.Fit, name))
                == inspect.signature(getattr(SqFitDouble, name)))


def test_gp_sq_integral_memoisation_and_invalidation(pkg):
    x, l = _samples()
    y = np.sqrt(2 * (l + 0.01))
    g = pkg.GP(pkg.GaussianKernel(1.0, 0.6), x, y, s=0.05)
    sq, var = g.sq_integral(0.3, 1.21)
    assert isinstance(sq, float) and isinstance(var, float) and var > 0 and sq > 0
    fit = g._fit
    n_calls = len(fit.calls)
    assert g.sq_integral([0.3], [[1.21]]) == (sq, var) and len(fit.calls) == n_calls  # memoised
    assert fit.calls[-1][0] == "sq_integral"
    assert g.sq_integral(0.0, 1.0) != (sq, var) and len(fit.calls) == n_calls + 1
    # the restatement is what comes back
    want = numpy_sqintegral(W_closed(x[None], x[None], 1.0, [0.6], [0.3], [[1.21]]),
                            Q_closed(x[None], 1.0, [0.6], [0.3], [[1.21]]),
                            gram_closed(x[None], x[None], 1.0, [0.6]) + 0.05 ** 2 * np.eye(13), y)
    assert abs(sq - want[0]) <= 1e-10 * want[0] and abs(var - want[1]) <= 1e-10 * want[5]
    # new parameters refit and recompute
    g.set_param("h", 1.3)
    assert g.sq_integral(0.3, 1.21) != (sq, var) and g._fit is fit and fit.calls[-1][4] == 1.3
    g.set_param("h", 1.0)
    assert g.sq_integral(0.3, 1.21) == (sq, var)
    # new targets: unlike ``integral``'s, this variance depends on them
    g.y = 2.0 * y
    sq2, var2 = g.sq_integral(0.3, 1.21)
    assert abs(sq2 - 4 * sq) <= 1e-9 * sq and abs(var2 - 4 * var) <= 1e-9 * var
    # append and remove
    g.append([0.1], [1.0])
    a = g.sq_integral(0.3, 1.21)
    assert a != (sq2, var2) and g._fit is fit and fit.calls[-2][0] == "append"
    g.remove([13])
    b = g.sq_integral(0.3, 1.21)
    assert fit.calls[-2][0] == "remove"
    assert abs(b[0] - sq2) <= 1e-9 * sq2 and abs(b[1] - var2) <= 1e-9 * var2


def test_gp_sq_integral_design_shapes_and_noisy(pkg):
    x, l = _samples()
    y = np.sqrt(2 * (l + 0.01))
    g = pkg.GP(pkg.GaussianKernel(1.0, 0.6), x, y, s=0.2)
    xo = np.linspace(-2.9, 2.9, 17)
    mu, cov = np.array([0.3]), np.array([[1.21]])
    idx = g.sq_integral_design(xo, 5, 0.3, 1.21)
    assert idx.shape == (5,) and idx.dtype == np.int64
    call = g._fit.calls[-1]
    assert call[:5] == ("sqdesign", 17, 5, 0.2 ** 2, 0.0)  # noisy by default: nugget = s^2
    assert np.array_equal(call[6], mu) and np.array_equal(call[7], cov)
    idx2, info = g.sq_integral_design(xo[None, :], 5, mu, cov, return_info=True)
    assert set(info) == {"gain", "zvar0", "resid", "resid_u"} and np.array_equal(idx2, idx)
    assert info["gain"].shape == (5,) and info["resid"].shape == (17,)
    assert abs(info["zvar0"] - g.sq_integral(mu, cov)[1]) <= 1e-14
    idx3, info3 = g.sq_integral_design(xo, 5, mu, cov, noisy=False, tol=1e-9, return_info=True)
    assert g._fit.calls[-1][3:5] == (0.0, 1e-9) and len(set(idx3.tolist())) == 5
    assert np.all(info3["resid"][idx3] == 0.0) and np.all(info3["resid_u"][idx3] == 0.0)
    idx4, info4 = g.sq_integral_design(xo, 5, mu, cov, tol=10.0, return_info=True)
    assert idx4.shape == (0,) and info4["gain"].shape == (0,)
    sc = g.sq_integral_scores(xo, mu, cov)
    assert sc.shape == (17,) and g._fit.calls[-1][2] == 1 and int(np.argmax(sc)) == idx[0]
    for e in ([], np.empty(0), np.empty((1, 0))):
        idx5, info5 = g.sq_integral_design(e, 3, mu, cov, return_info=True)
        assert idx5.shape == (0,) and idx5.dtype == np.int64
        assert abs(info5["zvar0"] - info["zvar0"]) <= 1e-14
        assert g.sq_integral_scores(e, mu, cov).shape == (0,)


def test_gp_sq_integral_argument_errors(pkg):
    x, l = _samples()
    g = pkg.GP(pkg.GaussianKernel(1.0, 0.6), x, np.sqrt(2 * (l + 0.01)), s=0.2)
    xo = np.array([0.1, 0.5, -2.0])
    for q in (0, -1, 4):
        with pytest.raises(ValueError):
            g.sq_integral_design(xo, q, 0.0, 1.0)
    for tol in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError):
            g.sq_integral_design(xo, 2, 0.0, 1.0, tol=tol)
    for mu, cov in (([0.0, 1.0], 1.0), (0.0, np.eye(2)), (np.nan, 1.0), (0.0, np.inf),
                    (0.0, -5.0)):
        with pytest.raises(ValueError):
            g.sq_integral(mu, cov)
        with pytest.raises(ValueError):
            g.sq_integral_design(xo, 2, mu, cov)
        with pytest.raises(ValueError):
            g.sq_integral_scores(xo, mu, cov)
    with pytest.raises(ValueError):
        g.sq_integral_design(np.zeros((2, 3)), 2, 0.0, 1.0)  # dimension mismatch with the fit
    assert g.sq_integral_design(xo, 3, 0.0, 1.0).shape == (3,)


def test_sqrt_bq_object(pkg):
    from bayesian_quadrature_amd.wsabi import SqrtBQ
    x, l = _samples()
    l = l + 0.05
    sb = SqrtBQ(x, l, pkg.GaussianKernel(1.0, 0.6), 0.05, 0.0, 1.0)
    assert sb.alpha0 == 0.8 * l.min()
    assert np.allclose(sb.gp.y, np.sqrt(2 * (l - sb.alpha0)), rtol=0, atol=0)
    with pytest.raises(ValueError):
        SqrtBQ(x, l, pkg.GaussianKernel(1.0, 0.6), 0.05, 0.0, 1.0, alpha0=l.min() * 1.01)
    with pytest.raises(ValueError):
        SqrtBQ(x, l[:-1], pkg.GaussianKernel(1.0, 0.6), 0.05, 0.0, 1.0)
    grid = np.linspace(-3.2, 3.2, 65)
    m, v = sb.gp.mean_var(grid)
    assert np.array_equal(sb.l_mean(grid), sb.alpha0 + 0.5 * m * m)
    assert np.allclose(sb.l_var(grid), m * m * np.maximum(v, 0), rtol=1e-15, atol=0)
    mean, var = sb.integral()
    sq, var2 = sb.gp.sq_integral([0.0], [[1.0]])
    assert mean == sb.alpha0 + 0.5 * sq and var == var2 and var > 0
    idx = sb.design(grid, 4)
    assert np.array_equal(idx, sb.gp.sq_integral_design(grid, 4, [0.0], [[1.0]]))
    # the acquisition and its gradient
    a = sb.acquisition(grid)
    pi = np.exp(-0.5 * grid ** 2) / np.sqrt(2 * np.pi)
    assert np.allclose(a, pi ** 2 * m * m * v, rtol=1e-13, atol=0)
    a2, da = sb.acquisition_grad(grid)
    assert np.allclose(a2, a, rtol=1e-12, atol=1e-300)
    e = 1e-6
    fd = (sb.acquisition(grid + e) - sb.acquisition(grid - e)) / (2 * e)
    assert np.max(np.abs(da - fd)) <= 1e-7 * np.max(np.abs(da))
    # observations at or above alpha0 are appended to the fit in place
    fit = sb.gp._fit
    sb.add_observation([0.15], [0.9])
    assert sb.gp._fit is fit and fit.calls[-1] == ("append", 1) and sb.x.shape == (14,)
    assert sb.gp.y[-1] == np.sqrt(2 * (0.9 - sb.alpha0)) and sb.integral() != (mean, var)
    # one below alpha0 moves alpha0 and refits
    a0 = sb.alpha0
    sb.add_observation([2.2], [0.5 * a0])
    assert sb.alpha0 == 0.8 * 0.5 * a0 and sb.gp._fit is not fit and sb.x.shape == (15,)
    assert np.allclose(sb.gp.y, np.sqrt(2 * (sb.l - sb.alpha0)), rtol=0, atol=0)
    assert np.all(sb.l_mean(grid) >= sb.alpha0)
    sb.add_observation([], [])
    assert sb.x.shape == (15,)


def test_sqrt_bq_survives_pickling(pkg):
    from bayesian_quadrature_amd.wsabi import SqrtBQ
    x, l = _samples()
    sb = SqrtBQ(x, l + 0.05, pkg.GaussianKernel(1.0, 0.6), 0.05, 0.2, 1.5)
    a = sb.integral()
    sb2 = pickle.loads(pickle.dumps(sb))
    assert sb2.gp._memoized == {} and sb2.gp._fit is None  # only data and parameters travel
    assert sb2.alpha0 == sb.alpha0 and sb2.integral() == a
    xo = np.linspace(-2, 2, 9)
    assert np.array_equal(sb2.design(xo, 3), sb.design(xo, 3))


def test_bq_sqrt_bq(pkg):
    import scipy.stats
    from bayesian_quadrature_amd.wsabi import SqrtBQ
    x = np.linspace(-5, 5, 9)
    l = scipy.stats.norm.pdf(x, 0, 1)
    bq = pkg.BQ(x, l, kernel=pkg.GaussianKernel, **OPTIONS)
    sb = bq.sqrt_bq((0.5, 1.3, 0.01))
    assert isinstance(sb, SqrtBQ) and sb.alpha0 == 0.8 * l.min()
    assert (sb.gp.K.h, sb.gp.K.w, sb.gp.s) == (0.5, 1.3, 0.01)
    assert np.array_equal(sb.x_mean, [OPTIONS["x_mean"]])
    assert np.array_equal(sb.x_cov, [[OPTIONS["x_var"]]])
    mean, var = sb.integral()
    assert mean >= sb.alpha0 and var > 0
    assert bq.sqrt_bq((0.5, 1.3, 0.01), alpha0=0.0).alpha0 == 0.0
    bqp = pkg.BQ(x, l, kernel=pkg.PeriodicKernel, **OPTIONS)
    with pytest.raises(NotImplementedError):
        bqp.sqrt_bq((0.5, 1.3, 0.01))
