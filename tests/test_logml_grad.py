"""The analytic gradient of the GP log marginal likelihood on the device (bq_gp_logml_grad,
engine.Fit.logml_grad, gp.GP.dloglh_dtheta, gp.GP.fit_MLII) against explicit CPU references."""
import numpy as np
import pytest

from bayesian_quadrature_amd import gp as gp_mod
from bayesian_quadrature_amd import util

pytestmark = pytest.mark.gpu


def _problem(n, d, s, seed, spread=3.0, w=None):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-spread, spread, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    if w is None:
        w = rs.uniform(0.6, 1.2, size=d) * spread / 3.0
    return x, y, 1.3, np.asarray(w, dtype=np.float64), float(s)


def _dK(x, h, w, s, K0):
    """dKxx / d theta in the order [h, w_1 .. w_d, s]."""
    d, n = x.shape
    out = [2.0 * K0 / h]
    for k in range(d):
        r2 = (x[k][:, None] - x[k][None, :]) ** 2
        out.append(K0 * (r2 / w[k] ** 2 - 1.0) / w[k])
    out.append(2.0 * s * np.eye(n))
    return out


def _reference(oracle, x, y, h, w, s):
    """(gradient, T): T_c = 1/2 sum (|a_i a_j| + |Kxx^-1_ij|) |dK_ij|, the size of its terms."""
    n = x.shape[1]
    L, a, _ = oracle.gp_fit(x, y, h, w, s)
    Kinv = oracle.cho_solve(L, np.eye(n))
    K0 = oracle.gram(x, h, w, 0.0)
    G = np.outer(a, a) - Kinv
    A = np.abs(np.outer(a, a)) + np.abs(Kinv)
    g, T = [], []
    for D in _dK(x, h, w, s, K0):
        g.append(0.5 * np.sum(G * D))
        T.append(0.5 * np.sum(A * np.abs(D)))
    return np.array(g), np.array(T)


# (n, d, s): npad 64 / 128 / 320 / 1024 / 1152 / 2048 -- both sides of the 256 -> 512 change of the
# sweep's block width at 1024 rows -- and all three noise levels
CASES = [
    (1, 1, 0.1), (9, 2, 0.0), (9, 3, 1e-3), (63, 1, 0.1), (64, 8, 1e-3), (65, 2, 0.1),
    (300, 3, 0.1), (300, 8, 0.0), (1000, 1, 0.1), (1000, 3, 1e-3), (1024, 8, 0.1),
    (1100, 3, 0.1), (2048, 1, 0.1), (2048, 2, 0.1),
]


@pytest.mark.parametrize("n,d,s", CASES)
def test_logml_grad_matches_cpu_reference(engine, oracle, n, d, s):
    x, y, h, w, s = _problem(n, d, s, seed=n + 10 * d)
    if s < 1e-2 or d == 8:  # points well apart: Kxx stays well conditioned with little noise
        w = w * 0.25
    Kxx = oracle.gram(x, h, w, s)
    assert np.linalg.cond(Kxx) <= 1e7
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        g = fit.logml_grad()
    finally:
        fit.close()
    gr, T = _reference(oracle, x, y, h, w, s)
    assert g.shape == (d + 2,)
    assert np.all(np.abs(g - gr) <= 1e-8 * T), (g, gr, T)


def _mp_reference(x, y, h, w, s):
    import mpmath as mp
    mp.mp.dps = 50
    d, n = x.shape
    c = mp.mpf(h) ** 2
    for k in range(d):
        c /= mp.sqrt(2 * mp.pi) * mp.mpf(w[k])

    def k0(i, j):
        q = mp.mpf(0)
        for k in range(d):
            q += (mp.mpf(x[k, i]) - mp.mpf(x[k, j])) ** 2 / (2 * mp.mpf(w[k]) ** 2)
        return c * mp.exp(-q)

    K0 = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            K0[i, j] = k0(i, j)
    Kxx = K0 + mp.mpf(s) ** 2 * mp.eye(n)
    Kinv = Kxx ** -1
    a = Kinv * mp.matrix([mp.mpf(v) for v in y])
    g = []
    for ch in range(d + 2):
        acc = mp.mpf(0)
        for i in range(n):
            for j in range(n):
                if ch == 0:
                    D = 2 * K0[i, j] / h
                elif ch <= d:
                    k = ch - 1
                    r2 = (mp.mpf(x[k, i]) - mp.mpf(x[k, j])) ** 2
                    D = K0[i, j] * (r2 / mp.mpf(w[k]) ** 2 - 1) / mp.mpf(w[k])
                else:
                    D = 2 * mp.mpf(s) if i == j else 0
                acc += (a[i] * a[j] - Kinv[i, j]) * D
        g.append(float(acc / 2))
    return np.array(g)


@pytest.mark.parametrize("n,d,s", [(7, 1, 0.0), (12, 2, 0.0), (12, 1, 0.2), (10, 3, 1e-2)])
def test_logml_grad_extended_precision(engine, oracle, n, d, s):
    x, y, h, w, s = _problem(n, d, s, seed=100 + n)
    w = w * 0.3
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        g = fit.logml_grad()
    finally:
        fit.close()
    _, T = _reference(oracle, x, y, h, w, s)
    gm = _mp_reference(x, y, h, w, s)
    assert np.all(np.abs(g - gm) <= 1e-10 * T), (g, gm, T)


def _alpha_bound(x, a, h, w, s, block=2048):
    """1/2 sum |a_i a_j| |dK_ij| per channel (d = 1): the alpha half of T_c, a lower bound of it."""
    n = x.shape[1]
    c = h * h / (np.sqrt(2 * np.pi) * w[0])
    T = np.zeros(3)
    aa = np.abs(a)
    for i0 in range(0, n, block):
        r2 = (x[0, i0:i0 + block, None] - x[0, None, :]) ** 2
        K0 = c * np.exp(-r2 / (2 * w[0] ** 2))
        A = aa[i0:i0 + block, None] * aa[None, :]
        T[0] += np.sum(A * 2.0 * K0 / h)
        T[1] += np.sum(A * K0 * np.abs(r2 / w[0] ** 2 - 1.0) / w[0])
    T[2] = np.sum(aa * aa) * 2.0 * s
    return 0.5 * T


@pytest.mark.parametrize("n", [4096, 16384])
def test_logml_grad_matches_central_difference_at_scale(engine, n):
    rs = np.random.RandomState(n)
    x = np.sort(rs.uniform(-5, 5, size=n))[None, :]
    y = np.sin(2 * x[0]) + 0.1 * rs.randn(n)
    theta = np.array([1.1, 0.05 if n > 4096 else 0.1, 0.1])
    fit = engine.gp_fit(x, y, theta[0], theta[1:2], theta[2])
    try:
        g = fit.logml_grad()
        a = fit.alpha()
        T = _alpha_bound(x, a, theta[0], theta[1:2], theta[2])

        def logml(t):
            fit.refit(t[0], t[1:2], t[2])
            return fit.logml

        for ch in range(3):
            # Richardson on two central differences: the h^2 term drops out
            def cd(step):
                e = np.zeros(3)
                e[ch] = step
                return (logml(theta + e) - logml(theta - e)) / (2 * step)

            st = 2e-3 * theta[ch]
            gfd = (4 * cd(st / 2) - cd(st)) / 3
            assert abs(g[ch] - gfd) <= 1e-6 * abs(g[ch]) + 1e-9 * T[ch], (ch, g, gfd, T)
    finally:
        fit.close()


def test_logml_grad_is_deterministic_and_isolated(engine):
    x, y, h, w, s = _problem(1000, 2, 0.1, seed=5)
    xo = np.random.RandomState(6).uniform(-3, 3, size=(2, 50))
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        lm0, a0 = fit.logml, fit.alpha()
        m0, v0, _ = fit.predict(xo)
        g1 = fit.logml_grad()
        g2 = fit.logml_grad()
        assert np.array_equal(g1, g2)
        assert fit.logml == lm0
        assert np.array_equal(fit.alpha(), a0)
        m1, v1, _ = fit.predict(xo)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
        # after a refit: the gradient of a fresh fit at the same parameters, same bits
        w2 = w * 1.3
        fit.refit(h * 0.9, w2, 0.05)
        g3 = fit.logml_grad()
        fresh = engine.gp_fit(x, y, h * 0.9, w2, 0.05)
        try:
            assert np.array_equal(g3, fresh.logml_grad())
        finally:
            fresh.close()
        assert not np.array_equal(g1, g3)
    finally:
        fit.close()


def test_logml_grad_status_rules(engine):
    x, y, h, w, s = _problem(100, 1, 0.1, seed=7)
    xd = np.concatenate([x, x], axis=1)
    yd = np.concatenate([y, y])
    fit = engine.gp_fit(xd, yd, h, w, s)
    try:
        with pytest.raises(np.linalg.LinAlgError):
            fit.refit(h, w, 0.0)  # repeated points without noise
        with pytest.raises(np.linalg.LinAlgError):
            fit.logml_grad()
        fit.refit(h, w, s)
        fit.logml_grad()
        fit.set_y(yd + 1.0)
        with pytest.raises(ValueError):
            fit.logml_grad()
    finally:
        fit.close()
    with pytest.raises(ValueError):
        fit.logml_grad()


def test_gp_dloglh_dtheta(engine):
    x, y, h, w, s = _problem(500, 1, 0.1, seed=8)
    g = gp_mod.GP(gp_mod.GaussianKernel(h, w[0]), x[0], y, s=s)
    d1 = g.dloglh_dtheta
    assert d1 is g.dloglh_dtheta
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        assert np.array_equal(d1, fit.logml_grad())
    finally:
        fit.close()
    g.set_param("w", w[0] * 1.1)
    d2 = g.dloglh_dtheta
    assert d2 is not d1 and not np.array_equal(d1, d2)
    g.y = y + 0.5
    d3 = g.dloglh_dtheta
    assert d3 is not d2 and not np.array_equal(d2, d3)


def test_gp_fit_MLII(engine, oracle):
    rs = np.random.RandomState(11)
    n = 1024
    x = np.sort(rs.uniform(-5, 5, size=n))
    h0, w0, s0 = 1.0, 0.7, 0.1
    K = oracle.gram(x[None, :], h0, np.array([w0]), s0)
    y = np.linalg.cholesky(K) @ rs.randn(n)
    start = (1.7 * h0, 0.6 * w0, 2 * s0)

    g = gp_mod.GP(gp_mod.GaussianKernel(start[0], start[1]), x, y, s=start[2])
    res = g.fit_MLII(["h", "w", "s"])
    assert res.success
    assert np.allclose(g.params, res.x, rtol=0, atol=0)
    ll_grad, nfev_grad = g.log_lh, util.LAST_OPT["nfev"]

    b = gp_mod.GP(gp_mod.GaussianKernel(start[0], start[1]), x, y, s=start[2])
    names = ("h", "w", "s")

    def logpdf(t):
        try:
            for nm, v in zip(names, t):
                b.set_param(nm, v)
            return b.log_lh
        except (ValueError, np.linalg.LinAlgError):
            return -np.inf

    lo = np.finfo(np.float64).tiny
    xb = util.find_good_parameters(logpdf, np.array(start), "L-BFGS-B",
                                   bounds=[(lo, None), (lo, None), (0.0, None)])
    assert xb is not None
    ll_fd, nfev_fd = logpdf(xb), util.LAST_OPT["nfev"]
    assert ll_grad >= ll_fd - 1e-8 * abs(ll_fd), (ll_grad, ll_fd)
    assert nfev_grad < nfev_fd, (nfev_grad, nfev_fd)
