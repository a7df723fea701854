"""CPU tests of the leave-one-out host plumbing: the formulas themselves in numpy (the gradient
against central differences of the value, the value against refits of the n - 1 others),
gp.GP.loo / log_loo / dlogloo_dtheta (order, memoisation, invalidation) and
gp.GP.fit_MLII(objective="loo"), over the oracle-backed engine double with a numpy LOO."""
import numpy as np
import pytest

from engine_double import EngineDouble, FitDouble
from test_logml_hess_host import numpy_logml_grad


def numpy_loo(o, x, y, h, w, s):
    """(mean, var, logpred, total) from the oracle's factor."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    w = np.atleast_1d(np.asarray(w, dtype=np.float64))
    n = x.shape[1]
    L, a, _ = o.gp_fit(x, y, h, w, s)
    k = np.diag(o.cho_solve(L, np.eye(n)))
    lp = 0.5 * np.log(k) - a * a / (2.0 * k) - 0.5 * np.log(2.0 * np.pi)
    return y - a / k, 1.0 / k, lp, float(np.sum(lp))


def numpy_loo_grad(o, x, y, h, w, s):
    """(total, [d/dh, d/dw_1 .. d/dw_d, d/ds]) with every matrix explicit:
    sum_i [a_i (Z_p a)_i - 1/2 (1 + a_i^2 / k_i) (Z_p Ki)_ii] / k_i, Z_p = Ki D_p."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    w = np.atleast_1d(np.asarray(w, dtype=np.float64))
    d, n = x.shape
    L, a, _ = o.gp_fit(x, y, h, w, s)
    Ki = o.cho_solve(L, np.eye(n))
    k = np.diag(Ki)
    K0 = o.gram(x, h, w, 0.0)
    D1 = [2.0 * K0 / h]
    for j in range(d):
        r2 = (x[j][:, None] - x[j][None, :]) ** 2
        D1.append(K0 * (r2 / w[j] ** 3 - 1.0 / w[j]))
    D1.append(2.0 * s * np.eye(n))
    g = []
    for D in D1:
        Z = Ki @ D
        g.append(np.sum((a * (Z @ a) - 0.5 * (1.0 + a * a / k) * np.sum(Z * Ki.T, axis=1)) / k))
    return numpy_loo(o, x, y, h, w, s)[3], np.array(g)


class LooFitDouble(FitDouble):
    def __init__(self, *args):
        self.calls = []
        FitDouble.__init__(self, *args)

    def _live(self):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")

    def logml_grad(self):
        self._live()
        self.calls.append("logml_grad")
        return numpy_logml_grad(self.o, self.x, self.y, self.h, self.w, self.s)

    def loo(self):
        self._live()
        self.calls.append("loo")
        return numpy_loo(self.o, self.x, self.y, self.h, self.w, self.s)

    def loo_grad(self):
        self._live()
        self.calls.append("loo_grad")
        return numpy_loo_grad(self.o, self.x, self.y, self.h, self.w, self.s)

    def _regrow(self, x, y):
        self.x, self.y = x, y
        self.n = self.y.shape[0]
        self._L, self._alpha, self.logml = self.o.gp_fit(self.x, self.y, self.h, self.w, self.s)

    def append(self, x_new, y_new):
        self._regrow(np.concatenate([np.ravel(self.x), np.ravel(x_new)]),
                     np.concatenate([self.y, np.ravel(y_new)]))

    def remove(self, idx):
        self._regrow(np.delete(np.ravel(self.x), idx), np.delete(self.y, idx))


class LooEngineDouble(EngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return LooFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def gpm(oracle):
    from bayesian_quadrature_amd import engine as eng_mod
    from bayesian_quadrature_amd import gp
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(LooEngineDouble(oracle), 0)
    yield gp
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _data(n=60, seed=3):
    rs = np.random.RandomState(seed)
    x = np.sort(rs.uniform(-4, 4, size=n))
    y = np.sin(x) + 0.1 * rs.randn(n)
    return x, y


def _data2(n=40, seed=4):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-3, 3, size=(2, n))
    return x, np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)


@pytest.mark.parametrize("two_d", [False, True])
def test_numpy_loo_gradient_matches_central_difference_of_the_value(oracle, two_d):
    if two_d:
        x, y = _data2()
        th = np.array([1.2, 0.8, 1.1, 0.2])
    else:
        x, y = _data()
        th = np.array([1.2, 0.8, 0.2])
    total, g = numpy_loo_grad(oracle, x, y, th[0], th[1:-1], th[-1])
    assert g.shape == th.shape
    assert total == numpy_loo(oracle, x, y, th[0], th[1:-1], th[-1])[3]
    for c in range(len(th)):
        e = np.zeros(len(th))
        e[c] = 1e-5 * th[c]
        v = [numpy_loo(oracle, x, y, t[0], t[1:-1], t[-1])[3] for t in (th + e, th - e)]
        fd = (v[0] - v[1]) / (2 * e[c])
        assert abs(fd - g[c]) <= 1e-5 * (1 + abs(g[c])), (c, fd, g[c])


def test_numpy_loo_matches_refits_of_the_others(oracle):
    """The check that does not share the formula: every point predicted by a fit of the rest."""
    x, y = _data(n=25)
    h, w, s = 1.2, 0.8, 0.2
    mean, var, lp, total = numpy_loo(oracle, x, y, h, w, s)
    K = oracle.gram(x[None, :], h, np.array([w]), s)
    for i in range(len(y)):
        o = np.delete(np.arange(len(y)), i)
        sol = np.linalg.solve(K[np.ix_(o, o)], np.stack([y[o], K[o, i]], axis=1))
        m, v = K[i, o] @ sol[:, 0], K[i, i] - K[i, o] @ sol[:, 1]
        assert abs(mean[i] - m) <= 1e-9 * (1 + abs(m)) and abs(var[i] - v) <= 1e-9 * v
        ref = -0.5 * np.log(2 * np.pi * v) - (y[i] - m) ** 2 / (2 * v)
        assert abs(lp[i] - ref) <= 1e-8 * (1 + abs(ref))
    assert total == float(np.sum(lp))


def test_numpy_loo_gradient_has_no_noise_entry_without_noise(oracle):
    x, y = _data(n=20)
    assert numpy_loo_grad(oracle, x, y, 1.2, 0.05, 0.0)[1][-1] == 0.0


def test_gp_loo_order_memoisation_and_invalidation(gpm, oracle):
    x, y = _data()
    g = gpm.GP(gpm.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    mean, var, lp = g.loo()
    ref = numpy_loo(oracle, x, y, 1.2, 0.8, 0.2)  # [h, w, s]
    assert all(np.array_equal(a, b) for a, b in zip((mean, var, lp), ref[:3]))
    assert g.log_loo == ref[3]
    again = g.loo()
    assert again[0] is mean and again[1] is var and again[2] is lp
    assert g._fit.calls.count("loo") == 1
    gr = g.dlogloo_dtheta
    assert gr.shape == (3,)
    assert np.array_equal(gr, numpy_loo_grad(oracle, x, y, 1.2, 0.8, 0.2)[1])
    assert g.dlogloo_dtheta is gr and g._fit.calls.count("loo_grad") == 1
    ll = g.log_lh
    assert g.loo()[2] is lp and g.dlogloo_dtheta is gr and g.log_lh == ll
    assert g._fit.calls.count("loo") == 1 and g._fit.calls.count("loo_grad") == 1

    g.set_param("h", 1.3)
    l2, g2 = g.log_loo, g.dlogloo_dtheta
    assert l2 != ref[3] and g2 is not gr and not np.array_equal(g2, gr)
    g.set_param("h", 1.3)  # no change: the memo stays
    assert g.dlogloo_dtheta is g2
    g.s = 0.25
    assert g.log_loo != l2 and g.dlogloo_dtheta is not g2
    g.y = y + 1.0
    l3, g3 = g.log_loo, g.dlogloo_dtheta
    assert l3 == numpy_loo(oracle, x, y + 1.0, 1.3, 0.8, 0.25)[3]
    g.append([0.1, 0.7], [0.2, 0.5])
    xa, ya = np.concatenate([x, [0.1, 0.7]]), np.concatenate([y + 1.0, [0.2, 0.5]])
    assert len(g.loo()[0]) == len(y) + 2
    assert g.log_loo == numpy_loo(oracle, xa, ya, 1.3, 0.8, 0.25)[3]
    g4 = g.dlogloo_dtheta
    assert g4 is not g3 and np.array_equal(g4, numpy_loo_grad(oracle, xa, ya, 1.3, 0.8, 0.25)[1])
    g.remove([5])
    xr, yr = np.delete(xa, 5), np.delete(ya, 5)
    assert len(g.loo()[2]) == len(y) + 1
    assert g.log_loo == numpy_loo(oracle, xr, yr, 1.3, 0.8, 0.25)[3]
    assert g.dlogloo_dtheta is not g4


def test_fit_MLII_on_loo_uses_the_loo_gradient_only(gpm):
    x, y = _data(n=80)
    g = gpm.GP(gpm.GaussianKernel(2.0, 0.5), x, y, s=0.3)
    start = g.log_loo
    res = g.fit_MLII(["h", "w", "s"], objective="loo")
    calls = g._fit.calls
    assert "loo_grad" in calls and "logml_grad" not in calls
    assert res.success and res.fun == -g.log_loo
    assert g.log_loo >= start
    assert np.array_equal(res.x, [g.K.h, g.K.w, g.s])
    assert np.max(np.abs(g.dlogloo_dtheta * res.x)) <= 1e-3 * len(y)


def test_fit_MLII_rejects_an_unknown_objective(gpm):
    x, y = _data()
    g = gpm.GP(gpm.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    with pytest.raises(ValueError):
        g.fit_MLII(["h"], objective="kfold")
    assert g.K.h == 1.2 and g._fit is None


def test_fit_MLII_default_objective_makes_the_calls_it_made(gpm):
    x, y = _data(n=80)
    runs = []
    for kw in ({}, {"objective": "log_lh"}):
        g = gpm.GP(gpm.GaussianKernel(2.0, 0.5), x, y, s=0.3)
        res = g.fit_MLII(["h", "w", "s"], **kw)
        runs.append((list(g._fit.calls), res.x, res.fun))
        assert "logml_grad" in g._fit.calls
        assert "loo" not in g._fit.calls and "loo_grad" not in g._fit.calls
        assert res.fun == -g.log_lh
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
