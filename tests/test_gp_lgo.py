"""Leave-group-out cross-validation of a resident fit on the device (bq_gp_lgo, bq_gp_lgo_grad,
engine.Fit.lgo / lgo_grad, gp.GP.lgo / log_lgo / dloglgo_dtheta / clusters,
fit_MLII(objective="lgo")) against explicit CPU references.

The tolerances follow test_gp_loo.py's recipe unchanged: the reference comes from Kxx^-1 and
Kxx^-1 y at 50 digits (n <= 65) or from the oracle's factor; a second float64 route with the
device's own algebra (Cholesky, Y = L^-T, Kxx^-1 = Y Y^T) gives, per quantity,
r = max |cpu - ref| / T with T the sum of the absolute values of the quantity's terms; the device
gets 100 max(r, 4 eps) T."""
import functools

import numpy as np
import pytest

from bayesian_quadrature_amd import gp as gp_mod
from test_gp_loo import _case, _check, _first_derivatives, _problem
from test_logml_hess import _mp_inverse

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
NAMES = ("mean", "var", "logpred", "total", "grad")


# ---- the groups ---------------------------------------------------------------------------
def _cut(perm, rs):
    out, i = [], 0
    while i < len(perm):
        b = rs.randint(1, 8)
        out.append(perm[i:i + b])
        i += b
    return out


def _scheme(n, name):
    """The groups of one scheme, seeded by n; None where the scheme does not apply."""
    rs = np.random.RandomState(n)
    if name == "singletons":
        return [np.array([i]) for i in range(n)]
    if name == "everything":  # one group of all points
        return [np.arange(n)] if n <= 64 else None
    if name == "blocks64":  # contiguous blocks of 64, the last one ragged
        return [np.arange(i, min(i + 64, n)) for i in range(0, n, 64)]
    if name == "scattered":  # a random permutation cut into sizes 1 .. 7
        return _cut(rs.permutation(n), rs)
    if name == "straddle":  # across a 64-row tile, a subset only, others never left out
        if n < 72:
            return None
        mid = n // 2 if not 58 <= n // 2 <= 70 else 71  # (n = 130: 65 is in the first group)
        return [np.arange(58, 71), np.array([0, n - 1, mid])]
    if name == "scattered64":  # one scattered group of 64
        return [rs.permutation(n)[:64]] if n >= 72 else None
    raise KeyError(name)


SCHEMES = ("singletons", "everything", "blocks64", "scattered", "straddle", "scattered64")
# (n, d, s) of test_gp_loo.py: npad 64 / 128 / 192 / 320, n on both sides of a 64 boundary, d = 8
# (the widest template), s = 0; and npad 1152 (several chunks of columns, more than 256 groups)
CASES = [(1, 1, 0.1), (2, 1, 0.1), (9, 2, 0.0), (63, 1, 0.1), (64, 8, 1e-3), (65, 2, 0.1),
         (130, 3, 0.1), (300, 3, 0.1)]
PARAMS = [(n, d, s, sch) for n, d, s in CASES for sch in SCHEMES if _scheme(n, sch) is not None]
PARAMS.append((1100, 3, 0.1, "scattered"))


# ---- the reference ------------------------------------------------------------------------
def _products(Ki, a, D1):
    """v_p = Ki D_p a and Ki D_p Ki over [h, w_1 .. w_d, s]."""
    return [Ki @ (D @ a) for D in D1], [Ki @ D @ Ki for D in D1]


def _lgo(Ki, a, y, V, M, groups):
    """The five quantities from Kxx^-1, Kxx^-1 y and the products, every matrix explicit."""
    mean, var, lp = [], [], []
    g = np.zeros(len(V))
    for B in groups:
        PBB = Ki[np.ix_(B, B)]
        S = np.linalg.inv(PBB)
        r = S @ a[B]
        mean.append(y[B] - r)
        var.append(np.diag(S).copy())
        lp.append(np.sum(np.log(np.diag(np.linalg.cholesky(PBB)))) - 0.5 * (a[B] @ r)
                  - len(B) * HALF_LOG_2PI)
        for p in range(len(V)):
            MB = M[p][np.ix_(B, B)]
            g[p] += r @ V[p][B] - 0.5 * (r @ MB @ r) - 0.5 * np.sum(S * MB)
    return {"mean": np.concatenate(mean), "var": np.concatenate(var), "logpred": np.array(lp),
            "total": float(np.sum(lp)), "grad": g}


def _lgo_sizes(Ki, a, y, Va, Ma, groups):
    """The sums of the absolute values of the terms of those quantities; Va, Ma: the products of
    the absolute values."""
    mean, var, lp = [], [], []
    g = np.zeros(len(Va))
    for B in groups:
        PBB = Ki[np.ix_(B, B)]
        S = np.abs(np.linalg.inv(PBB))
        aa = np.abs(a[B])
        r = S @ aa
        mean.append(np.abs(y[B]) + r)
        var.append(np.diag(S).copy())
        lp.append(np.sum(np.abs(np.log(np.diag(np.linalg.cholesky(PBB))))) + 0.5 * (aa @ r)
                  + len(B) * HALF_LOG_2PI)
        for p in range(len(Va)):
            MB = Ma[p][np.ix_(B, B)]
            g[p] += r @ Va[p][B] + 0.5 * (r @ MB @ r) + 0.5 * np.sum(S * MB)
    return {"mean": np.concatenate(mean), "var": np.concatenate(var), "logpred": np.array(lp),
            "total": float(np.sum(lp)), "grad": g}


def _matrices(oracle, x, y, h, w, s):
    """What every scheme of one problem shares: the reference's and the CPU route's Kxx^-1,
    Kxx^-1 y and products, and the products of the absolute values."""
    from scipy.linalg import solve_triangular
    d, n = x.shape
    K0 = oracle.gram(x, h, w, 0.0)
    D1 = _first_derivatives(x, h, w, s, K0)
    if n <= 65:
        Ki, a = _mp_inverse(x, y, h, w, s)
    else:
        L, a, _ = oracle.gp_fit(x, y, h, w, s)
        Ki = oracle.cho_solve(L, np.eye(n))
    ref = (Ki, a) + _products(Ki, a, D1)
    sizes = _products(np.abs(Ki), np.abs(a), [np.abs(D) for D in D1])
    # the device's own algebra in float64 on the CPU
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    Y = solve_triangular(Lc, np.eye(n), lower=True).T
    a2 = solve_triangular(Lc, solve_triangular(Lc, y, lower=True), lower=True, trans="T")
    Ki2 = Y @ Y.T
    cpu = (Ki2, a2) + _products(Ki2, a2, D1)
    return ref, sizes, cpu


def _reference(mats, y, groups, label=""):
    """(ref, T, tol), each a dict over NAMES."""
    (Ki, a, V, M), (Va, Ma), (Ki2, a2, V2, M2) = mats
    ref = _lgo(Ki, a, y, V, M, groups)
    T = _lgo_sizes(Ki, a, y, Va, Ma, groups)
    cpu = _lgo(Ki2, a2, y, V2, M2, groups)
    tol = {}
    for q in NAMES:
        t, e = np.atleast_1d(T[q]), np.atleast_1d(np.abs(cpu[q] - ref[q]))
        pos = t > 0
        r = float(np.max(e[pos] / t[pos]))
        tol[q] = MARGIN * max(r, 4 * EPS) * T[q]
        print("%s %s: r %.3g" % (label, q, r))
    # the bound cannot hide a wrong gradient entry or a wrong total
    pos = T["grad"] > 0
    assert np.all(tol["grad"][pos] <= 1e-2 * np.abs(ref["grad"][pos])), (tol["grad"], ref["grad"])
    assert tol["total"] <= 1e-2 * abs(ref["total"]), (tol["total"], ref["total"])
    return ref, T, tol


@functools.lru_cache(maxsize=None)
def _case_matrices(oracle, n, d, s):
    return _matrices(oracle, *_case(n, d, s))


@functools.lru_cache(maxsize=None)
def _case_reference(oracle, n, d, s, scheme):
    return _reference(_case_matrices(oracle, n, d, s), _case(n, d, s)[1], _scheme(n, scheme),
                      "n=%d d=%d s=%g %s" % (n, d, s, scheme))


def _value(fit, groups):
    return dict(zip(NAMES[:4], fit.lgo(groups)))


def _gradient(fit, groups):
    return dict(zip(("total", "grad"), fit.lgo_grad(groups)))


def _same(a, b):
    return all(np.array_equal(a[q], b[q]) for q in a)


def _device(engine, n, d, s, groups):
    x, y, h, w, s = _case(n, d, s)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        got, grad = _value(fit, groups), _gradient(fit, groups)
    finally:
        fit.close()
    T, G = sum(len(B) for B in groups), len(groups)
    assert got["mean"].shape == (T,) and got["var"].shape == (T,)
    assert got["logpred"].shape == (G,) and grad["grad"].shape == (d + 2,)
    assert grad["total"] == got["total"]
    got["grad"] = grad["grad"]
    return got


# ---- values and gradient ------------------------------------------------------------------
@pytest.mark.parametrize("n,d,s,scheme", PARAMS)
def test_lgo_and_its_gradient_match_cpu_reference(engine, oracle, n, d, s, scheme):
    got = _device(engine, n, d, s, _scheme(n, scheme))
    _check(got, *_case_reference(oracle, n, d, s, scheme), NAMES)


@pytest.mark.parametrize("n,d,s,scheme", [p for p in PARAMS if p[0] <= 130])
def test_lgo_matches_fits_of_the_remaining_points(engine, oracle, n, d, s, scheme):
    """The check that does not share the formula: every group predicted by a numpy fit of the
    points outside it (by the prior where the group is everything)."""
    x, y, h, w, s = _case(n, d, s)
    groups = _scheme(n, scheme)
    K = oracle.gram(x, h, w, s)
    mean, var, lp = [], [], []
    for B in groups:
        o = np.setdiff1d(np.arange(n), B)
        m, cov = np.zeros(len(B)), K[np.ix_(B, B)]
        if o.size:
            sol = np.linalg.solve(K[np.ix_(o, o)], np.column_stack([y[o], K[np.ix_(o, B)]]))
            m, cov = K[np.ix_(B, o)] @ sol[:, 0], cov - K[np.ix_(B, o)] @ sol[:, 1:]
        e = y[B] - m
        mean.append(m)
        var.append(np.diag(cov))
        lp.append(-np.sum(np.log(np.diag(np.linalg.cholesky(cov))))
                  - 0.5 * (e @ np.linalg.solve(cov, e)) - len(B) * HALF_LOG_2PI)
    want = {"mean": np.concatenate(mean), "var": np.concatenate(var), "logpred": np.array(lp)}
    got = _device(engine, n, d, s, groups)
    _, T, tol = _case_reference(oracle, n, d, s, scheme)
    _check(got, want, T, tol, ("mean", "var", "logpred"))


@pytest.mark.parametrize("n,d,s", CASES)
def test_lgo_of_singletons_is_loo(engine, oracle, n, d, s):
    x, y, h, w, s = _case(n, d, s)
    groups = _scheme(n, "singletons")
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        got = dict(_value(fit, groups), grad=fit.lgo_grad(groups)[1])
        want = dict(zip(NAMES[:4], fit.loo()), grad=fit.loo_grad()[1])
    finally:
        fit.close()
    _, T, tol = _case_reference(oracle, n, d, s, "singletons")
    _check(got, want, T, tol, NAMES)


@pytest.mark.parametrize("n,d,s", [c for c in CASES if c[0] <= 64])
def test_lgo_of_everything_is_the_marginal_likelihood(engine, oracle, n, d, s):
    x, y, h, w, s = _case(n, d, s)
    groups = _scheme(n, "everything")
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        got = dict(zip(("total", "grad"), fit.lgo_grad(groups)))
        want = {"total": fit.logml, "grad": fit.logml_grad()}
    finally:
        fit.close()
    _, T, tol = _case_reference(oracle, n, d, s, "everything")
    _check(got, want, T, tol, ("total", "grad"))


# ---- determinism and isolation ------------------------------------------------------------
def test_lgo_is_deterministic_and_isolated(engine, oracle):
    n = 300
    x, y, h, w, s = _problem(n, 2, 0.1, seed=5)
    xo = np.random.RandomState(6).uniform(-3, 3, size=(2, 50))
    for scheme in ("scattered", "blocks64"):
        groups = _scheme(n, scheme)
        fit = engine.gp_fit(x, y, h, w, s)
        hessian_first = engine.gp_fit(x, y, h, w, s)
        try:
            lm0, a0 = fit.logml, fit.alpha()
            m0, v0, _ = fit.predict(xo)
            g0 = fit.logml_grad()
            loo0 = fit.loo()
            # hessian_first: the Hessian and loo_grad, then LGO; fit: LGO, its gradient, then those
            H0 = hessian_first.logml_hess()
            lg0 = hessian_first.loo_grad()
            v1 = _value(fit, groups)
            assert _same(v1, _value(fit, groups))
            gr1 = _gradient(fit, groups)
            assert _same(gr1, _gradient(fit, groups))
            assert gr1["total"] == v1["total"]
            assert _same(v1, _value(fit, groups))
            assert _same(gr1, _gradient(hessian_first, groups))
            assert _same(v1, _value(hessian_first, groups))
            assert np.array_equal(fit.logml_hess(), H0)
            lg1 = fit.loo_grad()
            assert lg1[0] == lg0[0] and np.array_equal(lg1[1], lg0[1])
            assert _same(v1, _value(fit, groups)) and _same(gr1, _gradient(fit, groups))
            # other groups in between leave these groups' results alone
            fit.lgo_grad(_scheme(n, "straddle"))
            assert _same(v1, _value(fit, groups)) and _same(gr1, _gradient(fit, groups))
            assert fit.logml == lm0
            assert np.array_equal(fit.alpha(), a0)
            m1, vv1, _ = fit.predict(xo)
            assert np.array_equal(m0, m1) and np.array_equal(v0, vv1)
            assert np.array_equal(fit.logml_grad(), g0)
            assert all(np.array_equal(p, q) for p, q in zip(fit.loo(), loo0))
            assert np.array_equal(fit.logml_hess(), H0)
            # after a refit: LGO of a fresh fit at the same parameters, same bits
            w2 = w * 1.3
            fit.refit(h * 0.9, w2, 0.05)
            v3, gr3 = _value(fit, groups), _gradient(fit, groups)
            fresh = engine.gp_fit(x, y, h * 0.9, w2, 0.05)
            try:
                assert _same(v3, _value(fresh, groups)) and _same(gr3, _gradient(fresh, groups))
            finally:
                fresh.close()
            assert not np.array_equal(v1["logpred"], v3["logpred"]) and v1["total"] != v3["total"]
            assert not np.array_equal(gr1["grad"], gr3["grad"])
            # after an append and after a remove: LGO of a fresh fit of the resulting data,
            # within the bound measured for those data
            rs = np.random.RandomState(7)
            xn = rs.uniform(-3, 3, size=(2, 3))
            yn = np.sin(xn).sum(axis=0) + 0.1 * rs.randn(3)
            fit.refit(h, w, s)
            fit.lgo_grad(groups)
            fit.append(xn, yn)
            xa, ya = np.concatenate([x, xn], axis=1), np.concatenate([y, yn])
            _agrees_with_fresh(engine, oracle, fit, xa, ya, h, w, s, groups + [np.arange(n, n + 3)])
            fit.remove([150])
            xr, yr = np.delete(xa, 150, axis=1), np.delete(ya, 150)
            _agrees_with_fresh(engine, oracle, fit, xr, yr, h, w, s, _scheme(n + 2, scheme))
        finally:
            fit.close()
            hessian_first.close()


def _agrees_with_fresh(engine, oracle, fit, x, y, h, w, s, groups):
    got = dict(_value(fit, groups), **_gradient(fit, groups))
    fresh = engine.gp_fit(x, y, h, w, s)
    try:
        want = dict(_value(fresh, groups), **_gradient(fresh, groups))
    finally:
        fresh.close()
    assert got["mean"].shape == want["mean"].shape == (sum(len(B) for B in groups),)
    _, T, tol = _reference(_matrices(oracle, x, y, h, w, s), y, groups, "n=%d" % len(y))
    _check(got, want, T, tol, NAMES)


# ---- status rules -------------------------------------------------------------------------
def test_lgo_status_rules(engine):
    x, y, h, w, s = _problem(100, 1, 0.1, seed=7)
    fit = engine.gp_fit(x, y, h, w, s)
    ok = [[3, 4, 5], [99, 0]]
    bad = {
        "a group of 65": [list(range(65))],
        "an empty group": [[1, 2], []],
        "an index at -1": [[1, -1]],
        "an index at n": [[1, 100]],
        "a duplicate within a group": [[7, 8, 7]],
        "a duplicate across groups": [[7, 8], [9, 8]],
        "no group": [],
    }
    try:
        before = fit.lgo(ok), fit.lgo_grad(ok)
        for what, groups in bad.items():
            for call in (fit.lgo, fit.lgo_grad):
                with pytest.raises(ValueError):
                    call(groups)
                    pytest.fail(what)
        fit.lgo([list(range(64))])  # the cap itself
        after = fit.lgo(ok), fit.lgo_grad(ok)
        assert all(np.array_equal(p, q) for p, q in zip(before[0], after[0]))
        assert before[1][0] == after[1][0] and np.array_equal(before[1][1], after[1][1])
        fit.set_y(y + 1.0)
        for call in (fit.lgo, fit.lgo_grad):
            with pytest.raises(ValueError):
                call(ok)
    finally:
        fit.close()
    for call in (fit.lgo, fit.lgo_grad):
        with pytest.raises(ValueError):
            call(ok)
    # repeated points without noise: no valid factor
    xd, yd = np.concatenate([x, x], axis=1), np.concatenate([y, y])
    fit = engine.gp_fit(xd, yd, h, w, s)
    try:
        with pytest.raises(np.linalg.LinAlgError):
            fit.refit(h, w, 0.0)
        for call in (fit.lgo, fit.lgo_grad):
            with pytest.raises(np.linalg.LinAlgError):
                call(ok)
        fit.refit(h, w, s)
        fit.lgo(ok)
        fit.lgo_grad(ok)
    finally:
        fit.close()


def test_lgo_gradient_has_no_noise_entry_without_noise(engine):
    x, y, h, w, s = _case(9, 2, 0.0)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        for scheme in ("singletons", "everything", "scattered"):
            assert fit.lgo_grad(_scheme(9, scheme))[1][-1] == 0.0
    finally:
        fit.close()


# ---- gp.GP and an optimiser run -----------------------------------------------------------
def _clustered(oracle, n, seed):
    """n / 2 near-duplicate pairs of a draw from a GP."""
    rs = np.random.RandomState(seed)
    left = np.sort(rs.uniform(-5, 5, size=n // 2))
    x = np.sort(np.concatenate([left, left + 1e-3]))
    K = oracle.gram(x[None, :], 1.0, np.array([0.7]), 0.1)
    return x, np.linalg.cholesky(K) @ rs.randn(n)


def test_gp_lgo_log_lgo_and_dloglgo_dtheta(engine, oracle):
    x, y = _clustered(oracle, 256, 8)
    h, w, s = 1.2, 0.8, 0.1
    g = gp_mod.GP(gp_mod.GaussianKernel(h, w), x, y, s=s)
    groups = g.clusters(1e-2)
    assert np.array_equal(np.sort(np.concatenate(groups)), np.arange(256))
    assert 1 < len(groups) < 256 and max(len(B) for B in groups) <= 64
    l1, g1, p1 = g.log_lgo(groups), g.dloglgo_dtheta(groups), g.lgo(groups)
    assert g1.shape == (3,) and len(p1) == 3
    assert g.dloglgo_dtheta(groups) is g1 and g.log_lgo([list(B) for B in groups]) == l1
    assert all(a is b for a, b in zip(g.lgo(groups), p1))
    fit = engine.gp_fit(x[None, :], y, h, np.array([w]), s)
    try:
        mean, var, lp, total = fit.lgo(groups)
        total2, grad = fit.lgo_grad(groups)
    finally:
        fit.close()
    assert l1 == total == total2 and np.array_equal(g1, grad)
    assert all(np.array_equal(a, b) for a, b in zip(p1, (mean, var, lp)))

    def dropped(before):
        now = (g.log_lgo(groups), g.dloglgo_dtheta(groups))
        assert now[0] != before[0]
        assert now[1] is not before[1] and not np.array_equal(now[1], before[1])
        return now

    g.set_param("w", w * 1.1)
    now = dropped((l1, g1))
    g.y = y + 0.5 * np.cos(x)
    now = dropped(now)
    g.append([0.05, 1.5], [0.3, 0.8])
    now = dropped(now)
    g.remove([257])
    dropped(now)
    assert len(g.lgo(groups)[0]) == 256


def test_fit_MLII_on_lgo(engine, oracle):
    x, y = _clustered(oracle, 256, 11)
    g = gp_mod.GP(gp_mod.GaussianKernel(1.5, 1.0), x, y, s=0.2)
    groups = g.clusters(1e-2)
    start = g.log_lgo(groups)
    res = g.fit_MLII(["h", "w", "s"], objective="lgo", groups=groups)
    print("log_lgo %.6g -> %.6g at %s after %d evaluations"
          % (start, g.log_lgo(groups), res.x, res.nfev))
    assert res.fun == -g.log_lgo(groups)
    assert g.log_lgo(groups) >= start
