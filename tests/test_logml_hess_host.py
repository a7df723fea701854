"""CPU tests of the log-ML Hessian's host plumbing: the formula itself in numpy (against central
differences of the gradient and the scaling identity), gp.GP.d2loglh_dtheta2 (order, memoisation)
and gp.GP.hyper_cov, over the oracle-backed engine double with a numpy Hessian."""
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


def numpy_logml_hess(o, x, y, h, w, s):
    """H_pq = 1/2 sum(G o D_pq) - (D_p a)^T Ki (D_q a) + 1/2 tr(Ki D_p Ki D_q) over
    [h, w_1 .. w_d, s], every matrix explicit."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    w = np.atleast_1d(np.asarray(w, dtype=np.float64))
    d, n = x.shape
    L, a, _ = o.gp_fit(x, y, h, w, s)
    Ki = o.cho_solve(L, np.eye(n))
    K0 = o.gram(x, h, w, 0.0)
    G = np.outer(a, a) - Ki
    r2 = [(x[k][:, None] - x[k][None, :]) ** 2 for k in range(d)]
    u = [r2[k] / w[k] ** 3 - 1.0 / w[k] for k in range(d)]
    D1 = [2.0 * K0 / h] + [K0 * u[k] for k in range(d)] + [2.0 * s * np.eye(n)]
    P = d + 2
    Z = np.zeros((n, n))
    D2 = [[Z] * P for _ in range(P)]
    D2[0][0] = 2.0 * K0 / h ** 2
    for k in range(d):
        D2[0][1 + k] = D2[1 + k][0] = 2.0 * D1[1 + k] / h
        for l in range(d):
            D2[1 + k][1 + l] = K0 * (u[k] * u[l] + (k == l) * (1.0 / w[k] ** 2
                                                               - 3.0 * r2[k] / w[k] ** 4))
    D2[P - 1][P - 1] = 2.0 * np.eye(n)
    B = [Ki @ D for D in D1]
    v = [D @ a for D in D1]
    H = np.empty((P, P))
    for p in range(P):
        for q in range(P):
            H[p, q] = (0.5 * np.sum(G * D2[p][q]) - v[p] @ (Ki @ v[q])
                       + 0.5 * np.sum(B[p] * B[q].T))
    return H


class HessFitDouble(FitDouble):
    def logml_grad(self):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        return numpy_logml_grad(self.o, self.x, self.y, self.h, self.w, self.s)

    def logml_hess(self):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        self.hessians = getattr(self, "hessians", 0) + 1
        return numpy_logml_hess(self.o, self.x, self.y, self.h, self.w, self.s)

    def append(self, x_new, y_new):
        self.x = np.concatenate([np.ravel(self.x), np.ravel(x_new)])
        self.y = np.concatenate([self.y, np.ravel(y_new)])
        self.n = self.y.shape[0]
        self._L, self._alpha, self.logml = self.o.gp_fit(self.x, self.y, self.h, self.w, self.s)


class HessEngineDouble(EngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return HessFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def gpm(oracle):
    from bayesian_quadrature_amd import engine as eng_mod
    from bayesian_quadrature_amd import gp
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(HessEngineDouble(oracle), 0)
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
def test_numpy_hessian_matches_central_difference_of_the_gradient(oracle, two_d):
    if two_d:
        x, y = _data2()
        th = np.array([1.2, 0.8, 1.1, 0.2])
    else:
        x, y = _data()
        th = np.array([1.2, 0.8, 0.2])
    H = numpy_logml_hess(oracle, x, y, th[0], th[1:-1], th[-1])
    assert np.array_equal(H.shape, (len(th), len(th)))
    assert np.allclose(H, H.T, rtol=1e-12, atol=0)
    for c in range(len(th)):
        e = np.zeros(len(th))
        e[c] = 1e-5 * th[c]
        g = [numpy_logml_grad(oracle, x, y, t[0], t[1:-1], t[-1]) for t in (th + e, th - e)]
        col = (g[0] - g[1]) / (2 * e[c])
        assert np.all(np.abs(col - H[:, c]) <= 1e-5 * (1 + np.abs(H[:, c]))), (c, col, H[:, c])


# (without noise the points have to lie a few length scales apart for Kxx to be well conditioned)
@pytest.mark.parametrize("w,s", [(0.8, 0.2), (0.05, 0.0)])
def test_numpy_hessian_satisfies_the_scaling_identity(oracle, w, s):
    """Along (h, s) -> (c h, c s) the likelihood is -q / (2 c^2) - n log c + const, q = y^T a."""
    x, y = _data(n=30)
    h = 1.2
    assert np.linalg.cond(oracle.gram(x[None, :], h, np.array([w]), s)) <= 1e4
    H = numpy_logml_hess(oracle, x, y, h, w, s)
    _, a, _ = oracle.gp_fit(x[None, :], y, h, np.array([w]), s)
    n, q = len(y), float(y @ a)
    lhs = h * h * H[0, 0] + 2 * h * s * H[0, 2] + s * s * H[2, 2]
    assert abs(lhs - (n - 3 * q)) <= 1e-9 * (n + 3 * abs(q))


def test_d2loglh_dtheta2_order_and_memoisation(gpm, oracle):
    x, y = _data()
    g = gpm.GP(gpm.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    H1 = g.d2loglh_dtheta2
    assert H1.shape == (3, 3)
    assert np.array_equal(H1, numpy_logml_hess(oracle, x, y, 1.2, 0.8, 0.2))  # [h, w, s]
    assert g.d2loglh_dtheta2 is H1
    assert g._fit.hessians == 1
    ll, gr = g.log_lh, g.dloglh_dtheta
    assert g.d2loglh_dtheta2 is H1 and g.log_lh == ll and g.dloglh_dtheta is gr
    assert g._fit.hessians == 1
    g.set_param("h", 1.3)
    H2 = g.d2loglh_dtheta2
    assert H2 is not H1 and not np.array_equal(H1, H2)
    g.s = 0.25
    H3 = g.d2loglh_dtheta2
    assert H3 is not H2 and not np.array_equal(H2, H3)
    g.y = y + 1.0
    H4 = g.d2loglh_dtheta2
    assert H4 is not H3
    assert np.array_equal(H4, numpy_logml_hess(oracle, x, y + 1.0, 1.3, 0.8, 0.25))
    g.set_param("h", 1.3)  # no change: the memo stays
    assert g.d2loglh_dtheta2 is H4
    g.append([0.1, 0.7], [0.2, 0.5])
    H5 = g.d2loglh_dtheta2
    assert H5 is not H4
    xa, ya = np.concatenate([x, [0.1, 0.7]]), np.concatenate([y + 1.0, [0.2, 0.5]])
    assert np.array_equal(H5, numpy_logml_hess(oracle, xa, ya, 1.3, 0.8, 0.25))


def test_hyper_cov_validates_its_subset(gpm):
    x, y = _data()
    g = gpm.GP(gpm.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    for bad in (["q"], [], ["h", "h"], ["h", "w", "s", "x"]):
        with pytest.raises(ValueError):
            g.hyper_cov(bad)


def test_hyper_cov_raises_away_from_a_maximum(gpm, oracle):
    x, y = _data(n=80)
    H = numpy_logml_hess(oracle, x, y, 2.0, 0.5, 0.3)
    assert np.linalg.eigvalsh(H).max() > 0  # not a maximum: confirmed, not assumed
    g = gpm.GP(gpm.GaussianKernel(2.0, 0.5), x, y, s=0.3)
    with pytest.raises(np.linalg.LinAlgError):
        g.hyper_cov(["h", "w", "s"])
    assert g.K.h == 2.0 and g.K.w == 0.5 and g.s == 0.3


def test_hyper_cov_at_the_optimum(gpm):
    x, y = _data(n=80)
    g = gpm.GP(gpm.GaussianKernel(2.0, 0.5), x, y, s=0.3)
    assert g.fit_MLII(["h", "w", "s"]).success
    H = g.d2loglh_dtheta2
    C = g.hyper_cov(["h", "w", "s"])
    assert np.array_equal(C, C.T)
    assert np.allclose(C, np.linalg.inv(-H), rtol=1e-10, atol=0)
    assert np.all(np.linalg.eigvalsh(C) > 0)
    # a subset holds the others fixed: the block of -H, in the order asked for
    Csw = g.hyper_cov(["s", "w"])
    assert np.allclose(Csw, np.linalg.inv(-H[np.ix_([2, 1], [2, 1])]), rtol=1e-10, atol=0)
    assert g.hyper_cov(["w"])[0, 0] == -1.0 / H[1, 1]
