"""CPU tests of the posterior's derivatives in the hyper-parameters theta = [h, w_1 .. w_d, s]:
the closed form itself in numpy (against central differences of the oracle's mean and variance
over every parameter) and the host plumbing -- engine.Fit.predict_dtheta's contract as
gp.GP.dmean_dtheta / dvar_dtheta / mean_var_dtheta / mean_var_laplace use it -- over the
oracle-backed engine double with a numpy predict_dtheta.  test_predict_dtheta.py holds the device
to the same closed form."""
import functools
import inspect

import numpy as np
import pytest

from engine_double import EngineDouble
from test_logml_hess_host import HessFitDouble, numpy_logml_hess
from test_predict_grad_host import _norm


def _weights(x, xo, w):
    """g_jik = (xo_jk - x_ik)^2 / w_k^3 - 1 / w_k as [k, j, i]."""
    return (xo[:, :, None] - x[:, None, :]) ** 2 / w[:, None, None] ** 3 - 1.0 / w[:, None, None]


def _dk(x, K0, w, k):
    """D_k = K0 o (r_k^2 / w_k^3 - 1 / w_k)."""
    return K0 * ((x[k][:, None] - x[k][None, :]) ** 2 / w[k] ** 3 - 1.0 / w[k])


def closed_form(x, xo, h, w, s, k0, K, K0, a, u, z, beta=None, var=None):
    """(dmean, dvar), (d + 2) x M each, rows over [h, w_1 .. w_d, s].  K: the cross Gram (M x n);
    K0: the Gram of x without noise; a = Kxx^-1 y; u = Kxx^-1 a; z: d x n, row k = Kxx^-1 (D_k a);
    beta (M x n, row j = Kxx^-1 k_j) and var (M,): None leaves dvar None."""
    d, M = xo.shape
    G = _weights(x, xo, w)
    ku = K @ u
    dmean = np.empty((d + 2, M))
    dmean[0] = (2.0 * s * s / h) * ku
    for k in range(d):
        dmean[1 + k] = (K * G[k]) @ a - K @ z[k]
    dmean[d + 1] = (-2.0 * s) * ku
    if beta is None:
        return dmean, None
    bb = np.sum(beta * beta, axis=1)
    dvar = np.empty((d + 2, M))
    dvar[0] = (2.0 / h) * (var - s * s * bb)
    for k in range(d):
        q = np.sum((beta @ _dk(x, K0, w, k)) * beta, axis=1)
        dvar[1 + k] = -k0 / w[k] - 2.0 * np.sum(K * G[k] * beta, axis=1) + q
    dvar[d + 1] = (2.0 * s) * bb
    return dmean, dvar


def term_sizes(x, xo, h, w, s, k0, K, K0, a, u, z, beta):
    """(T_dmean, T_dvar), (d + 2) x M each: the norm products of the terms of every entry -- not the
    sums of |term|, which collapse to rounding noise at a query on a training point with s = 0,
    where beta_j is a unit vector (test_predict_grad_host.term_sizes has the same reason).
    var_j = k0 - k_j . beta_j counts as k0 + ||k_j|| ||beta_j||."""
    d, M = xo.shape
    G = _weights(x, xo, w)
    nk, nb = _norm(K), _norm(beta)
    Tm, Tv = np.empty((d + 2, M)), np.empty((d + 2, M))
    Tm[0] = (2.0 * s * s / h) * nk * _norm(u)
    Tm[d + 1] = (2.0 * s) * nk * _norm(u)
    Tv[0] = (2.0 / h) * (k0 + nk * nb + s * s * nb ** 2)
    Tv[d + 1] = (2.0 * s) * nb ** 2
    for k in range(d):
        nkg = _norm(K * G[k])
        Tm[1 + k] = nkg * _norm(a) + nk * _norm(z[k])
        Tv[1 + k] = k0 / w[k] + 2.0 * nkg * nb + nb * _norm(beta @ _dk(x, K0, w, k))
    return Tm, Tv


def numpy_pieces(o, x, y, h, w, s, xo, want_var=True):
    """The operands of closed_form / term_sizes from the oracle's factor, as a dict of their
    keyword names."""
    d, n = x.shape
    L, a, _ = o.gp_fit(x, y, h, w, s)
    K = np.ascontiguousarray(o.gram_cross(xo, x, h, w))
    K0 = np.ascontiguousarray(o.gram(x, h, w, 0.0))
    k0 = o.kernel_scale(d, h, w)
    u = o.cho_solve(L, a)
    z = np.array([o.cho_solve(L, _dk(x, K0, w, k) @ a) for k in range(d)])
    p = dict(k0=k0, K=K, K0=K0, a=a, u=u, z=z, beta=None, var=None)
    if want_var:
        p["beta"] = np.ascontiguousarray(o.cho_solve(L, K.T).T)
        p["var"] = k0 - np.sum(K * p["beta"], axis=1)
    return p


def numpy_predict_dtheta(o, x, y, h, w, s, xo, want_var=True):
    """(mean, var, dmean, dvar) from the oracle's factor; var and dvar None without want_var."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    xo = np.atleast_2d(np.asarray(xo, dtype=np.float64))
    w = np.atleast_1d(np.asarray(w, dtype=np.float64))
    p = numpy_pieces(o, x, y, h, w, s, xo, want_var)
    dmean, dvar = closed_form(x, xo, h, w, s, **p)
    return p["K"] @ p["a"], p["var"], dmean, dvar


class ThetaFitDouble(HessFitDouble):
    def __init__(self, *args):
        self.calls = []
        HessFitDouble.__init__(self, *args)

    def predict_dtheta(self, xo, want_var=True):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        xo = np.asarray(xo, dtype=np.float64)
        xo = xo[None, :] if xo.ndim == 1 else xo
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        self.calls.append(("predict_dtheta", want_var, self.n, self.h))
        return numpy_predict_dtheta(self.o, self.x, self.y, self.h, self.w, self.s, xo, want_var)

    def _regrow(self, x, y):
        self.x, self.y = x, y
        self.n = self.y.shape[0]
        self._L, self._alpha, self.logml = self.o.gp_fit(self.x, self.y, self.h, self.w, self.s)

    def append(self, x_new, y_new):
        self._regrow(np.concatenate([np.ravel(self.x), np.ravel(x_new)]),
                     np.concatenate([self.y, np.ravel(y_new)]))

    def remove(self, idx):
        self._regrow(np.delete(np.ravel(self.x), idx), np.delete(self.y, idx))


class ThetaEngineDouble(EngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return ThetaFitDouble(self.o, x, y, h, w, s)


def stands_in_for_the_product(test):
    """The numpy closed form and the double stand in for bq_gp_predict_dtheta and
    engine.Fit.predict_dtheta, with the same arguments: without those in the product there is
    nothing for them to stand in for, and the test fails."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        from bayesian_quadrature_amd import _lib, engine
        assert "bq_gp_predict_dtheta" in _lib.SIGNATURES
        assert _lib.SIGNATURES["bq_gp_predict_dtheta"] == _lib.SIGNATURES["bq_gp_predict_grad"]
        assert (inspect.signature(engine.Fit.predict_dtheta)
                == inspect.signature(ThetaFitDouble.predict_dtheta))
        return test(*args, **kwargs)
    return run


@pytest.fixture
def pkg(oracle):
    import bayesian_quadrature_amd as pkg
    from bayesian_quadrature_amd import engine as eng_mod
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(ThetaEngineDouble(oracle), 0)
    yield pkg
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _data(n=40, seed=3):
    rs = np.random.RandomState(seed)
    x = np.sort(rs.uniform(-3, 3, size=n))
    return x, np.sin(x) + 0.1 * rs.randn(n)


@pytest.mark.parametrize("d,s", [(1, 0.1), (2, 0.1), (2, 0.0)])
@stands_in_for_the_product
def test_closed_form_matches_central_differences_of_the_posterior(oracle, d, s):
    """Every parameter is differenced with the step 1e-5 (h and w are O(1); s is 0.1 or 0, and
    at s = 0 the two sides of the difference are the same function value, because only s^2
    enters).  Truncation is step^2 |f'''| / 6 ~ 1e-10 of an entry.  Rounding: a posterior from a
    factor of Kxx carries eps cond(Kxx) of its terms' size, and the difference divides it by the
    step: with cond(Kxx) <= 1e4, which the test asserts, 2.2e-16 x 1e4 / 1e-5 = 2.2e-7 T.  An
    error of sign, scale or index is O(T).  The bar 1e-5 T leaves a factor 45 above the first and
    five decades below the second.  At s = 0 the h row of dmean and the s rows of both are
    exactly 0.0 (T = 0 there); the differences they are compared with are then pure rounding
    noise, held to the same bar against the size of the mean's / the variance's own terms."""
    rs = np.random.RandomState(5 + d)
    n, M = 40, 7
    x = rs.uniform(-3, 3, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    h, w = 1.3, rs.uniform(0.6, 1.2, size=d)
    if s == 0.0:  # points well apart: Kxx stays well conditioned without noise
        w = w * 0.25
    assert np.linalg.cond(oracle.gram(x, h, w, s)) <= 1e4
    xo = rs.uniform(-3, 3, size=(d, M))
    xo[:, 0] = x[:, 0]  # a query on a training point
    mean, var, dmean, dvar = numpy_predict_dtheta(oracle, x, y, h, w, s, xo)
    L, a, _ = oracle.gp_fit(x, y, h, w, s)
    m0, v0 = oracle.gp_predict(x, h, w, L, a, xo)
    assert np.allclose(mean, m0, rtol=0, atol=1e-12 * np.abs(a).sum())
    assert np.allclose(var, v0, rtol=0, atol=1e-10)
    p = numpy_pieces(oracle, x, y, h, w, s, xo)
    p.pop("var")
    Tm, Tv = term_sizes(x, xo, h, w, s, **p)
    assert dmean.shape == dvar.shape == (d + 2, M)
    theta = np.concatenate([[h], w, [s]])
    step = 1e-5

    def posterior(t):
        t = np.abs(t)  # (s - step at s = 0: only s^2 enters)
        Lt, at, _ = oracle.gp_fit(x, y, t[0], t[1:-1], t[-1])
        return oracle.gp_predict(x, t[0], t[1:-1], Lt, at, xo)

    for c in range(d + 2):
        e = np.zeros(d + 2)
        e[c] = step
        (mp_, vp_), (mm_, vm_) = posterior(theta + e), posterior(theta - e)
        em = np.abs((mp_ - mm_) / (2 * step) - dmean[c])
        ev = np.abs((vp_ - vm_) / (2 * step) - dvar[c])
        live_m, live_v = Tm[c] > 0, Tv[c] > 0
        print("d=%d s=%g p=%d: worst error / T, dmean %.3g dvar %.3g"
              % (d, s, c, np.max(em[live_m] / Tm[c][live_m]) if live_m.any() else 0.0,
                 np.max(ev[live_v] / Tv[c][live_v]) if live_v.any() else 0.0))
        # (a row that is zero by construction, T = 0: the difference itself is only rounding
        # noise of the differenced mean / variance, whose terms have the size below)
        bar_m = np.where(live_m, Tm[c], _norm(p["K"]) * _norm(p["a"]))
        bar_v = np.where(live_v, Tv[c], p["k0"] + _norm(p["K"]) * _norm(p["beta"]))
        assert np.all(em <= 1e-5 * bar_m), (c, em, bar_m)
        assert np.all(ev <= 1e-5 * bar_v), (c, ev, bar_v)
    if s == 0.0:
        assert np.all(dmean[0] == 0.0) and np.all(dmean[d + 1] == 0.0)
        assert np.all(dvar[d + 1] == 0.0)
    else:
        assert np.all(dmean[[0, d + 1]] != 0.0) and np.all(dvar[d + 1] > 0.0)


@stands_in_for_the_product
def test_fit_contract_shapes_and_routes(oracle):
    x, y = _data()
    f = ThetaEngineDouble(oracle).gp_fit(x, y, 1.2, 0.8, 0.2)
    m, v, dm, dv = f.predict_dtheta(np.array([0.1, 0.5, -2.0]))
    assert m.shape == v.shape == (3,) and dm.shape == dv.shape == (3, 3)
    m2, v2, dm2, dv2 = f.predict_dtheta(np.array([[0.1, 0.5, -2.0]]), want_var=False)
    assert v2 is None and dv2 is None
    assert np.array_equal(m2, m) and np.array_equal(dm2, dm)
    with pytest.raises(ValueError):
        f.predict_dtheta(np.zeros((2, 3)))


@stands_in_for_the_product
def test_gp_derivatives_shapes_scalar_and_empty_input(pkg, oracle):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.array([0.1, 0.5, -2.0, x[3]])
    ref = numpy_predict_dtheta(oracle, x, y, 1.2, 0.8, 0.2, xo)
    dm, dv = g.dmean_dtheta(xo), g.dvar_dtheta(xo)
    assert dm.shape == dv.shape == (3, 4)
    assert np.array_equal(dm, ref[2]) and np.array_equal(dv, ref[3])
    got = g.mean_var_dtheta(xo)
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    assert np.allclose(got[0], g.mean(xo), rtol=0, atol=1e-12)
    assert np.allclose(got[1], g.var(xo), rtol=0, atol=1e-12)
    # the mean's derivatives take the route without a sweep
    assert [c[1] for c in g._fit.calls] == [False, True, True]
    # a scalar is one point (numpy sums one column in another order than four: n eps of the terms'
    # size, which is within 1e3 of the entries here)
    one = g.dmean_dtheta(0.1)
    assert one.shape == (3, 1) and np.allclose(one[:, 0], dm[:, 0], rtol=1e-10, atol=0)
    assert g.dvar_dtheta(0.1).shape == (3, 1)
    n_calls = len(g._fit.calls)
    empty = g.mean_var_dtheta(np.empty(0))
    assert empty[0].shape == empty[1].shape == (0,)
    for out in (g.dmean_dtheta([]), g.dvar_dtheta([])) + empty[2:]:
        assert out.shape == (3, 0) and out.dtype == np.float64
    assert len(g._fit.calls) == n_calls  # an empty query reaches no device


@stands_in_for_the_product
def test_gp_derivatives_follow_parameters_and_data(pkg, oracle):
    """After set_param, a new y, append and remove the fit is refreshed: nothing is stale."""
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.array([0.1, 0.5, -2.0])

    def check(x, y, h, w, s):
        ref = numpy_predict_dtheta(oracle, x, y, h, w, s, xo)
        got = g.mean_var_dtheta(xo)
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
        assert np.array_equal(g.dmean_dtheta(xo), ref[2])
        assert np.array_equal(g.dvar_dtheta(xo), ref[3])
        return got

    g0 = check(x, y, 1.2, 0.8, 0.2)
    g.set_param("h", 1.3)
    g1 = check(x, y, 1.3, 0.8, 0.2)
    assert not np.array_equal(g1[2], g0[2])
    assert g._fit.calls[-1][3] == 1.3  # the same fit, refitted
    g.set_param("w", 0.7)
    g.s = 0.25
    check(x, y, 1.3, 0.7, 0.25)
    g.y = y + 1.0
    check(x, y + 1.0, 1.3, 0.7, 0.25)
    g.append([0.1, 0.7], [0.2, 0.5])
    xa, ya = np.concatenate([x, [0.1, 0.7]]), np.concatenate([y + 1.0, [0.2, 0.5]])
    check(xa, ya, 1.3, 0.7, 0.25)
    assert g._fit.calls[-1][2] == len(y) + 2
    g.remove([5])
    check(np.delete(xa, 5), np.delete(ya, 5), 1.3, 0.7, 0.25)
    assert g._fit.calls[-1][2] == len(y) + 1


@stands_in_for_the_product
def test_mean_var_laplace_is_var_plus_the_quadratic_form(pkg, oracle):
    x, y = _data(n=60)
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    g.fit_MLII(["h", "w", "s"])
    th = [g.get_param(p) for p in ("h", "w", "s")]
    xo = np.array([0.1, 0.5, -2.0, 3.4])
    _, var, dm, _ = numpy_predict_dtheta(oracle, x, y, th[0], th[1], th[2], xo)
    H = numpy_logml_hess(oracle, x, y, th[0], th[1], th[2])
    for params in (["h", "w", "s"], ["w"], ["s", "h"]):
        idx = [("h", "w", "s").index(p) for p in params]
        C = np.linalg.inv(-H[np.ix_(idx, idx)])
        C = 0.5 * (C + C.T)
        assert np.array_equal(C, g.hyper_cov(params))
        extra = np.array([dm[idx, j] @ C @ dm[idx, j] for j in range(xo.size)])
        m, v = g.mean_var_laplace(xo, params)
        assert np.array_equal(m, g.mean(xo))
        assert np.all(extra > 0) and np.all(v > g.var(xo))
        # (var by the fit's own predict, which rounds apart from the closed form's by 1e-10)
        assert np.allclose(v, g.var(xo) + extra, rtol=1e-13, atol=0)
        assert np.allclose(v, var + extra, rtol=0, atol=1e-10)
    m, v = g.mean_var_laplace([], ["w"])
    assert m.shape == v.shape == (0,)
    # hyper_cov's own errors: bad names, and a point that is no maximum
    for bad in ([], ["x"], ["h", "h"]):
        with pytest.raises(ValueError):
            g.mean_var_laplace(xo, bad)
    g.set_param("w", 3.0 * th[1])
    g.set_param("h", 0.2 * th[0])
    with pytest.raises(np.linalg.LinAlgError):
        g.mean_var_laplace(xo, ["h", "w", "s"])
