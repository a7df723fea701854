"""Leave-one-out cross-validation of a resident fit on the device (bq_gp_loo, bq_gp_loo_grad,
engine.Fit.loo / loo_grad, gp.GP.loo / log_loo / dlogloo_dtheta, fit_MLII(objective="loo"))
against explicit CPU references.

The tolerances are measured, not fixed, as in test_logml_hess.py: the reference comes from
Kxx^-1 and Kxx^-1 y at 50 digits (n <= 65) or from the oracle's factor; a second float64 route
with the device's own algebra (Cholesky, Y = L^-T, Kxx^-1 = Y Y^T) gives, per quantity,
r = max |cpu - ref| / T with T the size of the quantity's terms; the device gets
100 max(r, 4 eps) T."""
import functools

import numpy as np
import pytest

from bayesian_quadrature_amd import gp as gp_mod
from test_logml_hess import _mp_inverse

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
NAMES = ("mean", "var", "logpred", "total", "grad")


def _problem(n, d, s, seed, spread=3.0, w=None):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-spread, spread, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    if w is None:
        w = rs.uniform(0.6, 1.2, size=d) * spread / 3.0
    return x, y, 1.3, np.asarray(w, dtype=np.float64), float(s)


def _case(n, d, s):
    x, y, h, w, s = _problem(n, d, s, seed=n + 10 * d)
    if s < 1e-2 or d == 8:  # points well apart: Kxx stays well conditioned with little noise
        w = w * 0.25
    return x, y, h, w, s


def _first_derivatives(x, h, w, s, K0):
    """D_p of Kxx over [h, w_1 .. w_d, s]."""
    d, n = x.shape
    D1 = [2.0 * K0 / h]
    for k in range(d):
        r2 = (x[k][:, None] - x[k][None, :]) ** 2
        D1.append(K0 * (r2 / w[k] ** 3 - 1.0 / w[k]))
    return D1 + [2.0 * s * np.eye(n)]


def _loo(Ki, a, y, s, D1, want_T=False):
    """The five quantities from Kxx^-1 and Kxx^-1 y, every matrix explicit; with want_T also
    the sizes of their terms."""
    k = np.diag(Ki).copy()
    lp = 0.5 * np.log(k) - a * a / (2.0 * k) - HALF_LOG_2PI
    B = [Ki @ D for D in D1[:-1]] + [2.0 * s * Ki]  # (D_s = 2 s I)
    c = 0.5 * (1.0 + a * a / k)
    g = [np.sum((a * (Ki @ (D @ a)) - c * np.sum(b * Ki.T, axis=1)) / k) for D, b in zip(D1, B)]
    val = {"mean": y - a / k, "var": 1.0 / k, "logpred": lp, "total": float(np.sum(lp)),
           "grad": np.array(g)}
    if not want_T:
        return val
    Tlp = 0.5 * np.abs(np.log(k)) + a * a / (2.0 * k) + HALF_LOG_2PI
    aKi, aa = np.abs(Ki), np.abs(a)
    Tg = [np.sum((aa * (aKi @ (np.abs(D) @ aa)) + c * np.sum(np.abs(b) * aKi.T, axis=1)) / k)
          for D, b in zip(D1, B)]
    T = {"mean": np.abs(y) + np.abs(a / k), "var": 1.0 / k, "logpred": Tlp,
         "total": float(np.sum(Tlp)), "grad": np.array(Tg)}
    return val, T


def _reference(oracle, x, y, h, w, s):
    """(ref, T, tol), each a dict over NAMES."""
    from scipy.linalg import solve_triangular
    d, n = x.shape
    K0 = oracle.gram(x, h, w, 0.0)
    D1 = _first_derivatives(x, h, w, s, K0)
    if n <= 65:
        Ki, a = _mp_inverse(x, y, h, w, s)
    else:
        L, a, _ = oracle.gp_fit(x, y, h, w, s)
        Ki = oracle.cho_solve(L, np.eye(n))
    ref, T = _loo(Ki, a, y, s, D1, want_T=True)
    # the device's own algebra in float64 on the CPU
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    Y = solve_triangular(Lc, np.eye(n), lower=True).T
    a2 = solve_triangular(Lc, solve_triangular(Lc, y, lower=True), lower=True, trans="T")
    cpu = _loo(Y @ Y.T, a2, y, s, D1)
    tol = {}
    for q in NAMES:
        t, e = np.atleast_1d(T[q]), np.atleast_1d(np.abs(cpu[q] - ref[q]))
        pos = t > 0
        r = float(np.max(e[pos] / t[pos]))
        tol[q] = MARGIN * max(r, 4 * EPS) * T[q]
        print("n=%d d=%d s=%g %s: r %.3g" % (n, d, s, q, r))
    # the bound cannot hide a wrong gradient entry or a wrong total
    pos = T["grad"] > 0
    assert np.all(tol["grad"][pos] <= 1e-2 * np.abs(ref["grad"][pos])), (tol["grad"], ref["grad"])
    assert tol["total"] <= 1e-2 * abs(ref["total"]), (tol["total"], ref["total"])
    return ref, T, tol


# (n, d, s): npad 64 / 128 / 192 / 320 / 1024 / 1152, n on both sides of a 64 boundary, d = 8
# (the widest template) and s = 0
CASES = [
    (1, 1, 0.1), (2, 1, 0.1), (9, 2, 0.0), (63, 1, 0.1), (64, 8, 1e-3), (65, 2, 0.1),
    (130, 3, 0.1), (300, 3, 0.1), (1000, 1, 0.1), (1100, 3, 0.1),
]


@functools.lru_cache(maxsize=None)
def _case_reference(oracle, n, d, s):
    return _reference(oracle, *_case(n, d, s))


def _check(got, ref, T, tol, names):
    for q in names:
        err, t = np.atleast_1d(np.abs(got[q] - ref[q])), np.atleast_1d(T[q])
        b, v = np.atleast_1d(tol[q]), np.atleast_1d(got[q])
        pos = t > 0
        print("worst |%s_dev - ref| / tol: %.3g" % (q, float(np.max(err[pos] / b[pos]))))
        assert np.all(err[pos] <= b[pos]), (q, got[q], ref[q], tol[q])
        assert np.all(v[~pos] == 0.0), (q, got[q], T[q])


def _value(fit):
    return dict(zip(NAMES[:4], fit.loo()))


def _gradient(fit):
    return dict(zip(("total", "grad"), fit.loo_grad()))


def _same(a, b):
    return all(np.array_equal(a[q], b[q]) for q in a)


@pytest.mark.parametrize("n,d,s", CASES)
def test_loo_matches_cpu_reference(engine, oracle, n, d, s):
    x, y, h, w, s = _case(n, d, s)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        got = _value(fit)
    finally:
        fit.close()
    assert all(got[q].shape == (n,) for q in NAMES[:3])
    _check(got, *_case_reference(oracle, n, d, s), NAMES[:4])


@pytest.mark.parametrize("n,d,s", CASES)
def test_loo_grad_matches_cpu_reference(engine, oracle, n, d, s):
    x, y, h, w, s = _case(n, d, s)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        got = _gradient(fit)
    finally:
        fit.close()
    assert got["grad"].shape == (d + 2,)
    _check(got, *_case_reference(oracle, n, d, s), ("total", "grad"))


@pytest.mark.parametrize("n,d,s", [c for c in CASES if c[0] <= 130])
def test_loo_matches_fits_of_the_other_points(engine, oracle, n, d, s):
    """The check that does not share the formula: every point predicted by a numpy fit of the
    n - 1 others."""
    x, y, h, w, s = _case(n, d, s)
    K = oracle.gram(x, h, w, s)
    mean, var = np.empty(n), np.empty(n)
    for i in range(n):
        o = np.delete(np.arange(n), i)
        sol = np.linalg.solve(K[np.ix_(o, o)], np.stack([y[o], K[o, i]], axis=1)) if n > 1 \
            else np.zeros((0, 2))
        mean[i], var[i] = K[i, o] @ sol[:, 0], K[i, i] - K[i, o] @ sol[:, 1]
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        got = _value(fit)
    finally:
        fit.close()
    _, T, tol = _case_reference(oracle, n, d, s)
    _check(got, {"mean": mean, "var": var}, T, tol, ("mean", "var"))


@pytest.mark.parametrize("n,d,s", [(300, 3, 0.1), (1100, 3, 0.1)])
def test_loo_tall_tile(engine, oracle, n, d, s, monkeypatch):
    """The products' 256 x 64 workgroup tile, which the large systems take, forced on systems
    whose npad (320, 1152) is no multiple of its 256 rows."""
    from bayesian_quadrature_amd.engine import Engine
    x, y, h, w, s = _case(n, d, s)
    monkeypatch.setenv("BQ_GEMM_TILE", "128")
    eng = Engine(0)
    try:
        fit = eng.gp_fit(x, y, h, w, s)
        try:
            got = _value(fit)
            grad = _gradient(fit)
        finally:
            fit.close()
    finally:
        eng.close()
    assert grad["total"] == got["total"]
    got["grad"] = grad["grad"]
    _check(got, *_case_reference(oracle, n, d, s), NAMES)


def test_loo_is_deterministic_and_isolated(engine, oracle):
    x, y, h, w, s = _problem(1000, 2, 0.1, seed=5)
    xo = np.random.RandomState(6).uniform(-3, 3, size=(2, 50))
    fit = engine.gp_fit(x, y, h, w, s)
    hessian_first = engine.gp_fit(x, y, h, w, s)
    try:
        lm0, a0 = fit.logml, fit.alpha()
        m0, v0, _ = fit.predict(xo)
        g0 = fit.logml_grad()
        # hessian_first: the Hessian, then LOO; fit: LOO, its gradient, then the Hessian
        H0 = hessian_first.logml_hess()
        v1 = _value(fit)
        assert _same(v1, _value(fit))
        gr1 = _gradient(fit)
        assert _same(gr1, _gradient(fit))
        assert gr1["total"] == v1["total"]
        assert _same(v1, _value(fit))
        assert _same(v1, _value(hessian_first))
        assert _same(gr1, _gradient(hessian_first))
        assert np.array_equal(fit.logml_hess(), H0)
        assert _same(v1, _value(fit)) and _same(gr1, _gradient(fit))
        assert fit.logml == lm0
        assert np.array_equal(fit.alpha(), a0)
        m1, vv1, _ = fit.predict(xo)
        assert np.array_equal(m0, m1) and np.array_equal(v0, vv1)
        assert np.array_equal(fit.logml_grad(), g0)
        # after a refit: LOO of a fresh fit at the same parameters, same bits
        w2 = w * 1.3
        fit.refit(h * 0.9, w2, 0.05)
        v3, gr3 = _value(fit), _gradient(fit)
        fresh = engine.gp_fit(x, y, h * 0.9, w2, 0.05)
        try:
            assert _same(v3, _value(fresh)) and _same(gr3, _gradient(fresh))
        finally:
            fresh.close()
        assert not np.array_equal(v1["logpred"], v3["logpred"]) and v1["total"] != v3["total"]
        assert not np.array_equal(gr1["grad"], gr3["grad"])
        # after an append and after a remove: LOO of a fresh fit of the resulting data, within
        # the bound measured for those data
        rs = np.random.RandomState(7)
        xn = rs.uniform(-3, 3, size=(2, 3))
        yn = np.sin(xn).sum(axis=0) + 0.1 * rs.randn(3)
        fit.refit(h, w, s)
        fit.loo_grad()
        fit.append(xn, yn)
        xa, ya = np.concatenate([x, xn], axis=1), np.concatenate([y, yn])
        _agrees_with_fresh(engine, oracle, fit, xa, ya, h, w, s, 1003)
        fit.remove([500])
        xr, yr = np.delete(xa, 500, axis=1), np.delete(ya, 500)
        _agrees_with_fresh(engine, oracle, fit, xr, yr, h, w, s, 1002)
    finally:
        fit.close()
        hessian_first.close()


def _agrees_with_fresh(engine, oracle, fit, x, y, h, w, s, n):
    got = dict(_value(fit), **_gradient(fit))
    assert all(got[q].shape == (n,) for q in NAMES[:3])
    fresh = engine.gp_fit(x, y, h, w, s)
    try:
        want = dict(_value(fresh), **_gradient(fresh))
    finally:
        fresh.close()
    _, T, tol = _reference(oracle, x, y, h, w, s)
    _check(got, want, T, tol, NAMES)


def test_loo_status_rules(engine):
    x, y, h, w, s = _problem(100, 1, 0.1, seed=7)
    xd = np.concatenate([x, x], axis=1)
    yd = np.concatenate([y, y])
    fit = engine.gp_fit(xd, yd, h, w, s)
    try:
        with pytest.raises(np.linalg.LinAlgError):
            fit.refit(h, w, 0.0)  # repeated points without noise
        for call in (fit.loo, fit.loo_grad):
            with pytest.raises(np.linalg.LinAlgError):
                call()
        fit.refit(h, w, s)
        fit.loo()
        fit.loo_grad()
        fit.set_y(yd + 1.0)
        for call in (fit.loo, fit.loo_grad):
            with pytest.raises(ValueError):
                call()
    finally:
        fit.close()
    for call in (fit.loo, fit.loo_grad):
        with pytest.raises(ValueError):
            call()


def test_gp_log_loo_and_dlogloo_dtheta(engine):
    x, y, h, w, s = _problem(500, 1, 0.1, seed=8)
    g = gp_mod.GP(gp_mod.GaussianKernel(h, w[0]), x[0], y, s=s)
    l1, g1, p1 = g.log_loo, g.dlogloo_dtheta, g.loo()
    assert g1.shape == (3,) and len(p1) == 3
    assert g.log_loo is l1 and g.dlogloo_dtheta is g1
    assert all(a is b for a, b in zip(g.loo(), p1))
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        mean, var, lp, total = fit.loo()
        total2, grad = fit.loo_grad()
    finally:
        fit.close()
    assert l1 == total == total2 and np.array_equal(g1, grad)
    assert all(np.array_equal(a, b) for a, b in zip(p1, (mean, var, lp)))

    def dropped(before):
        now = (g.log_loo, g.dlogloo_dtheta)
        assert now[0] != before[0]
        assert now[1] is not before[1] and not np.array_equal(now[1], before[1])
        return now

    g.set_param("w", w[0] * 1.1)
    now = dropped((l1, g1))
    g.y = y + 0.5 * np.cos(x[0])
    now = dropped(now)
    g.append([0.05, 1.5], [0.3, 0.8])
    now = dropped(now)
    assert len(g.loo()[0]) == 502
    g.remove([10])
    dropped(now)
    assert len(g.loo()[0]) == 501


def test_loo_finds_an_outlier(engine):
    rs = np.random.RandomState(12)
    n, j = 200, 77
    x = np.sort(rs.uniform(-3, 3, size=n))
    y = np.sin(x) + 0.05 * rs.randn(n)
    y[j] += 5.0
    g = gp_mod.GP(gp_mod.GaussianKernel(1.0, 0.7), x, y, s=0.1)
    assert int(np.argmin(g.loo()[2])) == j
    before = g.log_loo / n
    g.remove([j])
    assert len(g.loo()[2]) == n - 1
    assert g.log_loo / (n - 1) > before


def test_fit_MLII_on_loo(engine, oracle):
    rs = np.random.RandomState(11)
    n = 512
    x = np.sort(rs.uniform(-5, 5, size=n))
    K = oracle.gram(x[None, :], 1.0, np.array([0.7]), 0.1)
    y = np.linalg.cholesky(K) @ rs.randn(n)
    g = gp_mod.GP(gp_mod.GaussianKernel(1.5, 1.0), x, y, s=0.2)
    start = g.log_loo
    res = g.fit_MLII(["h", "w", "s"], objective="loo")
    print("log_loo %.6g -> %.6g at %s after %d evaluations" % (start, g.log_loo, res.x, res.nfev))
    assert res.fun == -g.log_loo
    assert g.log_loo >= start
    # the optimiser's own convergence scale, not an accuracy claim
    assert np.sum(np.abs(g.dlogloo_dtheta * res.x)) < 1e-3 * n
