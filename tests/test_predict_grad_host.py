"""CPU tests of the posterior's gradients at the query points: the closed form itself in numpy
(against central differences of the oracle's mean and variance) and the host plumbing --
engine.Fit.predict_grad's contract as gp.GP.dmean_dx / dvar_dx / mean_var_grad and
BQ.l_mean_grad / l_var_grad use it -- over the oracle-backed engine double with a numpy
predict_grad.  test_predict_grad.py holds the device to the same closed form."""
import numpy as np
import pytest

from engine_double import EngineDouble, FitDouble


def closed_form(K, x, xo, w, alpha, beta):
    """(dmean, dvar), d x M each, from the cross Gram K (M x n), alpha = Kxx^-1 y and
    beta (M x n, row j = Kxx^-1 k_j); either of alpha, beta may be None."""
    E = (x[:, None, :] - xo[:, :, None]) / w[:, None, None] ** 2  # e_jik as [k, j, i]
    KE = K[None, :, :] * E
    dmean = None if alpha is None else KE @ alpha
    dvar = None if beta is None else -2.0 * np.sum(KE * beta[None, :, :], axis=2)
    return dmean, dvar


def term_sizes(K, x, xo, w, alpha, beta):
    """(T_dmean, T_dvar), d x M each: the norm products ||k_j o e_jk|| ||alpha|| and
    2 ||k_j o e_jk|| ||beta_j|| -- not the sum of |term|, which collapses to rounding noise at a
    query on a training point with s = 0, where beta_j is a unit vector."""
    E = (x[:, None, :] - xo[:, :, None]) / w[:, None, None] ** 2
    return _norm(K[None, :, :] * E) * _norm(alpha), 2.0 * _norm(K[None, :, :] * E) * _norm(beta)[None, :]


def _norm(a):
    """2-norm along the last axis, scaled by the largest entry: a query far from every training
    point has k_ji ~ 1e-175, whose squares underflow."""
    big = np.max(np.abs(a), axis=-1, keepdims=True)
    scale = np.where(big > 0, big, 1.0)
    return (big * np.sqrt(np.sum((a / scale) ** 2, axis=-1, keepdims=True)))[..., 0]


def numpy_predict_grad(o, x, y, h, w, s, xo, want_var=True):
    """(mean, var, dmean, dvar) from the oracle's factor; var and dvar None without want_var."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    xo = np.atleast_2d(np.asarray(xo, dtype=np.float64))
    w = np.atleast_1d(np.asarray(w, dtype=np.float64))
    L, a, _ = o.gp_fit(x, y, h, w, s)
    K = np.ascontiguousarray(o.gram_cross(xo, x, h, w))
    beta = np.ascontiguousarray(o.cho_solve(L, K.T).T) if want_var else None
    dmean, dvar = closed_form(K, x, xo, w, a, beta)
    mean = K @ a
    var = o.kernel_scale(x.shape[0], h, w) - np.sum(K * beta, axis=1) if want_var else None
    return mean, var, dmean, dvar


class GradFitDouble(FitDouble):
    def __init__(self, *args):
        self.calls = []
        FitDouble.__init__(self, *args)

    def predict_grad(self, xo, want_var=True):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        xo = np.asarray(xo, dtype=np.float64)
        xo = xo[None, :] if xo.ndim == 1 else xo
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        self.calls.append(("predict_grad", want_var, self.n, self.h))
        return numpy_predict_grad(self.o, self.x, self.y, self.h, self.w, self.s, xo, want_var)

    def _regrow(self, x, y):
        self.x, self.y = x, y
        self.n = self.y.shape[0]
        self._L, self._alpha, self.logml = self.o.gp_fit(self.x, self.y, self.h, self.w, self.s)

    def append(self, x_new, y_new):
        self._regrow(np.concatenate([np.ravel(self.x), np.ravel(x_new)]),
                     np.concatenate([self.y, np.ravel(y_new)]))

    def remove(self, idx):
        self._regrow(np.delete(np.ravel(self.x), idx), np.delete(self.y, idx))


class GradEngineDouble(EngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return GradFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def pkg(oracle):
    import bayesian_quadrature_amd as pkg
    from bayesian_quadrature_amd import engine as eng_mod
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(GradEngineDouble(oracle), 0)
    yield pkg
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _data(n=40, seed=3):
    rs = np.random.RandomState(seed)
    x = np.sort(rs.uniform(-3, 3, size=n))
    return x, np.sin(x) + 0.1 * rs.randn(n)


@pytest.mark.parametrize("d", [1, 2])
def test_closed_form_matches_central_differences_of_the_posterior(oracle, d):
    """Step 1e-5 x 3.0 (the box half-width): truncation h^2 |f'''| / 6 ~ 1e-10, rounding
    eps |f| / h ~ 1e-11, and any error of sign, scale or index is O(T) -- the bar 1e-6 T leaves
    four decades either way."""
    rs = np.random.RandomState(5 + d)
    n, M = 40, 7
    x = rs.uniform(-3, 3, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    h, w, s = 1.3, rs.uniform(0.6, 1.2, size=d), 0.1
    xo = rs.uniform(-3, 3, size=(d, M))
    xo[:, 0] = x[:, 0]  # a query on a training point
    mean, var, dmean, dvar = numpy_predict_grad(oracle, x, y, h, w, s, xo)
    L, a, _ = oracle.gp_fit(x, y, h, w, s)
    m0, v0 = oracle.gp_predict(x, h, w, L, a, xo)
    assert np.allclose(mean, m0, rtol=0, atol=1e-12 * np.abs(a).sum())
    assert np.allclose(var, v0, rtol=0, atol=1e-10)
    K = np.ascontiguousarray(oracle.gram_cross(xo, x, h, w))
    Tm, Tv = term_sizes(K, x, xo, w, a, oracle.cho_solve(L, K.T).T)
    assert dmean.shape == dvar.shape == (d, M)
    step = 1e-5 * 3.0
    for k in range(d):
        e = np.zeros((d, 1))
        e[k] = step
        mp_, vp_ = oracle.gp_predict(x, h, w, L, a, xo + e)
        mm_, vm_ = oracle.gp_predict(x, h, w, L, a, xo - e)
        em = np.abs((mp_ - mm_) / (2 * step) - dmean[k])
        ev = np.abs((vp_ - vm_) / (2 * step) - dvar[k])
        print("d=%d k=%d: worst error / T, dmean %.3g dvar %.3g"
              % (d, k, np.max(em / Tm[k]), np.max(ev / Tv[k])))
        assert np.all(em <= 1e-6 * Tm[k]), (k, em, Tm[k])
        assert np.all(ev <= 1e-6 * Tv[k]), (k, ev, Tv[k])


def test_fit_contract_shapes_and_routes(oracle):
    x, y = _data()
    f = GradEngineDouble(oracle).gp_fit(x, y, 1.2, 0.8, 0.2)
    m, v, dm, dv = f.predict_grad(np.array([0.1, 0.5, -2.0]))
    assert m.shape == v.shape == (3,) and dm.shape == dv.shape == (1, 3)
    m2, v2, dm2, dv2 = f.predict_grad(np.array([[0.1, 0.5, -2.0]]), want_var=False)
    assert v2 is None and dv2 is None
    assert np.array_equal(m2, m) and np.array_equal(dm2, dm)
    with pytest.raises(ValueError):
        f.predict_grad(np.zeros((2, 3)))


def test_gp_gradients_shapes_and_empty_input(pkg, oracle):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.array([0.1, 0.5, -2.0, x[3]])
    ref = numpy_predict_grad(oracle, x, y, 1.2, 0.8, 0.2, xo)
    dm, dv = g.dmean_dx(xo), g.dvar_dx(xo)
    assert dm.shape == dv.shape == (4,)
    assert np.array_equal(dm, ref[2][0]) and np.array_equal(dv, ref[3][0])
    m, v, dm2, dv2 = g.mean_var_grad(xo)
    assert all(np.array_equal(a, b) for a, b in zip((m, v, dm2, dv2),
                                                    (ref[0], ref[1], ref[2][0], ref[3][0])))
    assert np.allclose(m, g.mean(xo), rtol=0, atol=1e-12)
    assert np.allclose(v, g.var(xo), rtol=0, atol=1e-12)
    # the mean's gradient takes the route without a sweep
    assert [c[1] for c in g._fit.calls] == [False, True, True]
    # a scalar is one point
    assert g.dmean_dx(0.1).shape == (1,) and abs(g.dmean_dx(0.1)[0] - dm[0]) <= 1e-13 * abs(dm[0])
    n_calls = len(g._fit.calls)
    for out in (g.dmean_dx([]), g.dvar_dx([])) + g.mean_var_grad(np.empty(0)):
        assert out.shape == (0,) and out.dtype == np.float64
    assert len(g._fit.calls) == n_calls  # an empty query reaches no device


def test_gp_gradients_follow_parameters_and_data(pkg, oracle):
    """After set_param, a new y, append and remove the fit is refreshed: nothing is stale."""
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.array([0.1, 0.5, -2.0])

    def check(x, y, h, w, s):
        ref = numpy_predict_grad(oracle, x, y, h, w, s, xo)
        got = g.mean_var_grad(xo)
        assert np.array_equal(got[2], ref[2][0]) and np.array_equal(got[3], ref[3][0])
        assert np.array_equal(g.dmean_dx(xo), ref[2][0])
        assert np.array_equal(g.dvar_dx(xo), ref[3][0])
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


OPTIONS = {
    "n_candidate": 10, "x_mean": 0.0, "x_var": 10.0, "candidate_thresh": 0.5,
    "optim_method": "L-BFGS-B",
}


def _bq(pkg):
    import scipy.stats
    np.random.seed(8728)
    x = np.linspace(-5, 5, 9)
    bq = pkg.BQ(x, scipy.stats.norm.pdf(x, 0, 1), kernel=pkg.GaussianKernel, **OPTIONS)
    bq.init(params_tl=(15, 2, 0), params_l=(0.2, 1.3, 0))
    return bq


def test_bq_l_mean_grad_is_the_second_gp_s(pkg):
    bq = _bq(pkg)
    xq = np.linspace(-4.3, 4.4, 11)
    assert np.array_equal(bq.l_mean_grad(xq), bq.gp_l.dmean_dx(xq))
    step = 1e-5
    fd = (bq.l_mean(xq + step) - bq.l_mean(xq - step)) / (2 * step)
    assert np.allclose(bq.l_mean_grad(xq), fd, rtol=1e-6, atol=1e-9)


def test_bq_l_var_grad_product_rule_differences_and_clamp(pkg, monkeypatch):
    bq = _bq(pkg)
    xq = np.linspace(-4.3, 4.4, 11)
    g = bq.l_var_grad(xq)
    assert g.shape == xq.shape
    _, v, _, dv = bq.gp_log_l.mean_var_grad(xq)
    m, _, dm, _ = bq.gp_l.mean_var_grad(xq)
    clamped = v * m ** 2 < 0
    expect = np.where(clamped, 0.0, dv * m ** 2 + 2.0 * v * m * dm)
    assert np.array_equal(g, expect)
    # against central differences of l_var, where a step stays clear of the clamp
    step = 1e-5
    lp, lm = bq.l_var(xq + step), bq.l_var(xq - step)
    free = (lp > 0) & (lm > 0) & ~clamped
    assert free.sum() >= 6
    fd = (lp - lm) / (2 * step)
    scale = np.abs(dv) * m ** 2 + 2.0 * np.abs(v * m * dm) + 1e-9 * bq.l_var(xq).max() / step
    assert np.all(np.abs(g - fd)[free] <= 1e-5 * scale[free]), (g, fd)

    # where l_var clamps to 0 the gradient is exactly 0: a log-GP whose variance comes out
    # negative at some points (as rounding makes it on training points without noise)
    real = bq.gp_log_l.mean_var_grad
    sign = np.where(np.arange(xq.size) % 3 == 0, -1.0, 1.0)

    def some_negative(x):
        m_, v_, dm_, dv_ = real(x)
        return m_, v_ * sign, dm_, dv_ * sign

    monkeypatch.setattr(bq.gp_log_l, "mean_var_grad", some_negative)
    monkeypatch.setattr(bq.gp_log_l, "var", lambda x: real(x)[1] * sign)
    g2 = bq.l_var_grad(xq)
    neg = (v * sign) * m ** 2 < 0
    assert neg.any() and (~neg).any()
    assert np.all(g2[neg] == 0.0) and np.all(bq.l_var(xq)[neg] == 0.0)
    assert np.array_equal(g2[~neg], g[~neg])


def test_bq_gradients_raise_on_the_approximate_branch(pkg):
    import scipy.stats
    x = np.linspace(-3, 3, 5)
    bq = pkg.BQ(x, scipy.stats.norm.pdf(x, 0, 1), kernel=pkg.PeriodicKernel, **OPTIONS)
    assert bq.options["use_approx"]
    for fn in (bq.l_mean_grad, bq.l_var_grad):
        with pytest.raises(NotImplementedError):
            fn(np.array([0.1, 0.2]))
