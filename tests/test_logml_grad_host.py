"""CPU tests of the log-ML gradient's host plumbing: gp.GP.dloglh_dtheta (order, memoisation),
gp.GP.fit_MLII and the exact-gradient route of util.find_good_parameters, over the oracle-backed
engine double with a numpy gradient."""
import numpy as np
import pytest

from engine_double import EngineDouble, FitDouble


def numpy_logml_grad(o, x, y, h, w, s):
    """[d/dh, d/dw_1 .. d/dw_d, d/ds] of the log marginal likelihood from the oracle's factor."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    w = np.atleast_1d(np.asarray(w, dtype=np.float64))
    d, n = x.shape
    L, a, _ = o.gp_fit(x, y, h, w, s)
    G = np.outer(a, a) - o.cho_solve(L, np.eye(n))
    K0 = o.gram(x, h, w, 0.0)
    g = [np.sum(G * K0) / h]
    for k in range(d):
        r2 = (x[k][:, None] - x[k][None, :]) ** 2
        g.append(np.sum(G * K0 * (r2 / w[k] ** 2 - 1.0)) / (2.0 * w[k]))
    g.append(s * np.trace(G))
    return np.array(g)


class GradFitDouble(FitDouble):
    def logml_grad(self):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        self.grads = getattr(self, "grads", 0) + 1
        return numpy_logml_grad(self.o, self.x, self.y, self.h, self.w, self.s)


class GradEngineDouble(EngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return GradFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def gpm(oracle):
    from bayesian_quadrature_amd import engine as eng_mod
    from bayesian_quadrature_amd import gp
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(GradEngineDouble(oracle), 0)
    yield gp
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _data(n=60, seed=3):
    rs = np.random.RandomState(seed)
    x = np.sort(rs.uniform(-4, 4, size=n))
    y = np.sin(x) + 0.1 * rs.randn(n)
    return x, y


def test_numpy_gradient_matches_central_difference(oracle):
    x, y = _data()
    th = np.array([1.2, 0.8, 0.2])
    g = numpy_logml_grad(oracle, x, y, th[0], th[1], th[2])
    for c in range(3):
        e = np.zeros(3)
        e[c] = 1e-5 * th[c]
        f = [oracle.gp_fit(x[None, :], y, t[0], t[1:2], t[2])[2] for t in (th + e, th - e)]
        assert abs((f[0] - f[1]) / (2 * e[c]) - g[c]) <= 1e-6 * (1 + abs(g[c]))


def test_dloglh_dtheta_order_and_memoisation(gpm, oracle):
    x, y = _data()
    g = gpm.GP(gpm.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    d1 = g.dloglh_dtheta
    assert d1.shape == (3,)
    assert np.array_equal(d1, numpy_logml_grad(oracle, x, y, 1.2, 0.8, 0.2))  # [h, w, s]
    assert g.dloglh_dtheta is d1
    assert g._fit.grads == 1
    ll = g.log_lh
    assert g.dloglh_dtheta is d1 and g.log_lh == ll
    g.set_param("h", 1.3)
    d2 = g.dloglh_dtheta
    assert d2 is not d1 and not np.array_equal(d1, d2)
    g.s = 0.25
    d3 = g.dloglh_dtheta
    assert d3 is not d2
    g.y = y + 1.0
    d4 = g.dloglh_dtheta
    assert d4 is not d3
    assert np.array_equal(d4, numpy_logml_grad(oracle, x, y + 1.0, 1.3, 0.8, 0.25))
    g.set_param("h", 1.3)  # no change: the memo stays
    assert g.dloglh_dtheta is d4


def test_fit_MLII_reaches_the_optimum(gpm):
    x, y = _data(n=80)
    g = gpm.GP(gpm.GaussianKernel(2.0, 0.5), x, y, s=0.3)
    res = g.fit_MLII(["h", "w", "s"])
    assert res.success
    assert np.array_equal(g.params, res.x)
    # every evaluation scipy counted was one gradient of the (test double's) fit, and nothing else
    # asked for one
    assert res.attempts == 1 and g._fit.grads == res.nfev
    assert np.all(np.abs(g.dloglh_dtheta) <= 1e-4 * (1 + abs(g.log_lh)))
    # a subset: s stays where it is
    g2 = gpm.GP(gpm.GaussianKernel(2.0, 0.5), x, y, s=0.3)
    g2.fit_MLII(["w"])
    assert g2.s == 0.3 and g2.K.h == 2.0
    assert abs(g2.dloglh_dtheta[1]) <= 1e-4 * (1 + abs(g2.log_lh))
    with pytest.raises(ValueError):
        g2.fit_MLII(["q"])


def test_fit_MLII_raises_without_an_optimum(gpm, monkeypatch):
    from bayesian_quadrature_amd import util
    x, y = _data()
    g = gpm.GP(gpm.GaussianKernel(1.0, 1.0), x, y, s=0.2)
    monkeypatch.setattr(util, "MIN", np.inf)
    with pytest.raises(RuntimeError):
        g.fit_MLII(["h"], ntry=2)
    assert g.K.h == 1.0


def test_find_good_parameters_with_exact_gradient():
    from bayesian_quadrature_amd import util
    c = np.array([1.5, -0.5, 2.0])
    S = np.array([[2.0, 0.3, 0.0], [0.3, 1.0, 0.2], [0.0, 0.2, 3.0]])
    calls = []

    def f(x):
        r = x - c
        return -0.5 * r @ S @ r + 4.0

    def fg(x):
        calls.append(1)
        r = x - c
        return f(x), -(S @ r)

    x = util.find_good_parameters(f, np.zeros(3), "L-BFGS-B", logpdf_grad=fg)
    assert np.allclose(x, c, atol=1e-6)
    assert util.LAST_OPT["success"] and util.LAST_OPT["nfev"] == len(calls)
    # bounds reach scipy
    xb = util.find_good_parameters(f, np.zeros(3), "L-BFGS-B", logpdf_grad=fg,
                                   bounds=[(None, None), (0.0, None), (None, None)])
    assert xb[1] >= 0.0 and abs(xb[1]) <= 1e-8
