"""Gradients of the posterior mean and variance at the query points on the device
(bq_gp_predict_grad, engine.Fit.predict_grad: both routes) against explicit CPU references.

The tolerances are measured, not fixed, as in test_logml_hess.py and test_gp_loo.py: the
reference comes from Kxx^-1, alpha, the cross Gram and the sums at 50 digits (n <= 65) or from the
oracle's factor; a second float64 route with the device's own algebra (Cholesky, the explicit
Y = L^-T, V = K(xo, x) Y, beta = V Y^T, alpha = Y Y^T y) gives, per quantity,
r = max |cpu - ref| / T, and the device gets 100 max(r, 4 eps) T.  T is the norm product
||k_j o e_jk|| ||alpha|| (dmean) and 2 ||k_j o e_jk|| ||beta_j|| (dvar), not the sum of |term|: at
a query on a training point with s = 0, beta_j is a unit vector and the term sum collapses to
rounding noise.  The first min(M // 4, n) queries are training points exactly: there the true
dvar is ~ 0 at small s, and beta cancels."""
import ctypes as C
import functools

import numpy as np
import pytest

from engine_env import engine_env
from test_predict_grad_host import closed_form, term_sizes

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0
NAMES = ("mean", "dmean", "dvar")


def _problem(n, d, s, seed, spread=3.0, w=None):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-spread, spread, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    if w is None:
        w = rs.uniform(0.6, 1.2, size=d) * spread / 3.0
    return x, y, 1.3, np.asarray(w, dtype=np.float64), float(s)


def _case(n, d, s, M):
    x, y, h, w, s = _problem(n, d, s, seed=n + 10 * d)
    if s < 1e-2 or d == 8:  # points well apart: Kxx stays well conditioned with little noise
        w = w * 0.25
    xo = np.random.RandomState(1000 + n).uniform(-3.3, 3.3, size=(d, M))
    on = min(M // 4, n)
    xo[:, :on] = x[:, :on]
    return x, y, h, w, s, np.asfortranarray(xo), on


def _mp_reference(x, y, h, w, s, xo):
    """(K, alpha, beta, mean, dmean, dvar) with Kxx^-1, alpha, the cross Gram and every sum at 50
    digits (the construction of test_logml_hess._mp_inverse, rounded only at the end)."""
    import mpmath as mp
    mp.mp.dps = 50
    d, n = x.shape
    M = xo.shape[1]
    X = [[mp.mpf(float(x[k, i])) for i in range(n)] for k in range(d)]
    XO = [[mp.mpf(float(xo[k, j])) for j in range(M)] for k in range(d)]
    W = [mp.mpf(float(w[k])) for k in range(d)]
    c = mp.mpf(h) ** 2
    for k in range(d):
        c /= mp.sqrt(2 * mp.pi) * W[k]

    def kern(p, q):
        return c * mp.exp(-sum((p[k] - q[k]) ** 2 / (2 * W[k] ** 2) for k in range(d)))

    Kxx = mp.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):
            Kxx[i, j] = Kxx[j, i] = kern([X[k][i] for k in range(d)], [X[k][j] for k in range(d)])
        Kxx[i, i] += mp.mpf(s) ** 2
    Ki = Kxx ** -1
    a = Ki * mp.matrix([mp.mpf(float(v)) for v in y])
    K = mp.matrix(M, n)
    for j in range(M):
        for i in range(n):
            K[j, i] = kern([XO[k][j] for k in range(d)], [X[k][i] for k in range(d)])
    B = K * Ki  # row j = (Kxx^-1 k_j)^T
    mean = np.empty(M)
    dmean, dvar = np.empty((d, M)), np.empty((d, M))
    for j in range(M):
        mean[j] = float(sum(K[j, i] * a[i] for i in range(n)))
        for k in range(d):
            e = [(X[k][i] - XO[k][j]) / W[k] ** 2 for i in range(n)]
            dmean[k, j] = float(sum(K[j, i] * e[i] * a[i] for i in range(n)))
            dvar[k, j] = float(-2 * sum(K[j, i] * e[i] * B[j, i] for i in range(n)))

    def arr(m_, r, c_):
        return np.array([[float(m_[i, j]) for j in range(c_)] for i in range(r)])

    return arr(K, M, n), np.array([float(a[i]) for i in range(n)]), arr(B, M, n), mean, dmean, dvar


def _reference(oracle, x, y, h, w, s, xo, on):
    """(ref, T, tol), each a dict over NAMES; prints r per quantity."""
    from scipy.linalg import solve_triangular
    d, n = x.shape
    M = xo.shape[1]
    if n <= 65:
        K, a, B, mean, dmean, dvar = _mp_reference(x, y, h, w, s, xo)
    else:
        L, a, _ = oracle.gp_fit(x, y, h, w, s)
        K = np.ascontiguousarray(oracle.gram_cross(xo, x, h, w))
        B = np.ascontiguousarray(oracle.cho_solve(L, K.T).T)
        mean = K @ a
        dmean, dvar = closed_form(K, x, xo, w, a, B)
    ref = {"mean": mean, "dmean": dmean, "dvar": dvar}
    Tm, Tv = term_sizes(K, x, xo, w, a, B)
    T = {"mean": np.abs(K) @ np.abs(a), "dmean": Tm, "dvar": Tv}
    # the device's own algebra in float64 on the CPU
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    Y = solve_triangular(Lc, np.eye(n), lower=True).T
    Kc = np.ascontiguousarray(oracle.gram_cross(xo, x, h, w))
    V = Kc @ Y
    Bc = V @ Y.T
    ac = Y @ (Y.T @ y)
    cm, cv = closed_form(Kc, x, xo, w, ac, Bc)
    cpu = {"mean": Kc @ ac, "dmean": cm, "dvar": cv}
    tol = {}
    for q in NAMES:
        pos = T[q] > 0
        r = float(np.max((np.abs(cpu[q] - ref[q])[pos]) / T[q][pos])) if pos.any() else 0.0
        tol[q] = MARGIN * max(r, 4 * EPS) * T[q]
        print("n=%d d=%d s=%g M=%d %s: r %.3g" % (n, d, s, M, q, r))
    # the bound cannot hide a wrong entry: away from the training points every entry of both
    # gradients is at least a hundred bounds large; on them dvar is ~ 0 and only dmean is
    assert np.all(tol["dmean"] <= 1e-2 * np.abs(ref["dmean"])), (tol["dmean"], ref["dmean"])
    assert np.all(tol["dvar"][:, on:] <= 1e-2 * np.abs(ref["dvar"][:, on:])), \
        (tol["dvar"][:, on:], ref["dvar"][:, on:])
    return ref, T, tol


# (n, d, s, M): npad 64 / 128 / 192 / 320 / 1024 / 1088, n on both sides of a 64 boundary, M on
# both sides of the 16-row workgroup and the 64-row padding, d = 8 (the widest template), s = 0,
# and in the last case (Mp = 1024, npad = 1088: no small route on 256 CUs) the fused backward
# sweep, where every other case takes the product loop
CASES = [
    (1, 1, 0.1, 1), (9, 2, 0.0, 17), (63, 1, 0.1, 64), (64, 8, 1e-3, 15), (65, 2, 0.1, 65),
    (130, 3, 0.1, 16), (300, 3, 0.0, 63), (300, 1, 0.1, 300), (1000, 1, 0.1, 64),
    (1050, 1, 0.1, 1000),
]


@functools.lru_cache(maxsize=None)
def _case_reference(oracle, n, d, s, M):
    return _reference(oracle, *_case(n, d, s, M))


def _check(got, ref, T, tol, names):
    for q in names:
        err = np.abs(got[q] - ref[q])
        pos = T[q] > 0
        if pos.any():
            print("worst |%s_dev - ref| / tol: %.3g" % (q, float(np.max(err[pos] / tol[q][pos]))))
        assert np.all(err[pos] <= tol[q][pos]), (q, got[q], ref[q], tol[q])
        assert np.all(got[q][~pos] == 0.0), (q, got[q], T[q])


def _full(engine, oracle, n, d, s, M):
    x, y, h, w, s, xo, on = _case(n, d, s, M)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        mean, var, dmean, dvar = fit.predict_grad(xo)
        pm, pv, _ = fit.predict(xo)
    finally:
        fit.close()
    assert mean.shape == var.shape == (M,) and dmean.shape == dvar.shape == (d, M)
    _check({"dmean": dmean, "dvar": dvar}, *_case_reference(oracle, n, d, s, M),
           ("dmean", "dvar"))
    # the sweep and the row reductions are bq_gp_predict's own
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)


def _mean_route(engine, oracle, n, d, s, M):
    x, y, h, w, s, xo, on = _case(n, d, s, M)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        mean, var, dmean, dvar = fit.predict_grad(xo, want_var=False)
    finally:
        fit.close()
    assert var is None and dvar is None
    assert mean.shape == (M,) and dmean.shape == (d, M)
    _check({"mean": mean, "dmean": dmean}, *_case_reference(oracle, n, d, s, M),
           ("mean", "dmean"))


@pytest.mark.parametrize("n,d,s,M", CASES)
def test_full_route_against_reference(engine, oracle, n, d, s, M):
    _full(engine, oracle, n, d, s, M)


@pytest.mark.parametrize("n,d,s,M", CASES)
def test_mean_route_against_reference(engine, oracle, n, d, s, M):
    _mean_route(engine, oracle, n, d, s, M)


@pytest.mark.parametrize("d", range(1, 9))
def test_every_dimension(engine, oracle, d):
    _full(engine, oracle, 20, d, 0.1, 5)
    _mean_route(engine, oracle, 20, d, 0.1, 5)


def _same(a, b):
    return all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(a, b))


def test_same_bits_twice(engine):
    for n, d, s, M in ((130, 3, 0.1, 16), (300, 1, 0.1, 300)):
        x, y, h, w, s, xo, _ = _case(n, d, s, M)
        fit = engine.gp_fit(x, y, h, w, s)
        try:
            a, b = fit.predict_grad(xo), fit.predict_grad(xo)
            assert all(v is not None for v in a) and _same(a, b)
            a, b = fit.predict_grad(xo, want_var=False), fit.predict_grad(xo, want_var=False)
            assert _same(a, b)
        finally:
            fit.close()


def _beyond_direct(n, d, M):
    """predict_direct_ok's rule (fit.hip): the cross Gram reads the points out of the mapped
    staging npad / 64 times, and does so only up to 4 MiB of such reads."""
    npad = -(-n // 64) * 64
    return d * M * 8 * (npad // 64) > 4 << 20


def _both_routes(eng, x, y, h, w, s, xo, with_predict=False):
    fit = eng.gp_fit(x, y, h, w, s)
    try:
        out = fit.predict_grad(xo) + fit.predict_grad(xo, want_var=False)
        return out + fit.predict(xo)[:2] if with_predict else out
    finally:
        fit.close()


def test_staging_routes(engine, oracle):
    """The three ways a call's points go in and its results come out give the same bits: the
    kernels on the mapped staging itself (the full route up to predict_direct_ok's limit), one
    copy kernel each way (the mean route, and the full route beyond the limit) and the copy engine
    (every route of an engine with BQ_SOLVE_KCOPY=0).  Two small cases with Mp != M and npad != n,
    and the smallest shape beyond the limit at d = 8, n = 1000: M = 4100 (Mp = 4160, a partly
    filled last block).  There mean and var are also predict's bits, and the first and the last 64
    queries -- a query's results do not depend on the other queries -- meet the reference under the
    module's measured bound."""
    with engine_env({"BQ_SOLVE_KCOPY": "0"}) as eng0:
        for n, d, s, M in ((130, 3, 0.1, 16), (300, 1, 0.1, 300)):
            assert not _beyond_direct(n, d, M)
            x, y, h, w, s, xo, _ = _case(n, d, s, M)
            a, b = (_both_routes(eng, x, y, h, w, s, xo) for eng in (engine, eng0))
            assert all(a[k] is not None for k in (0, 1, 2, 3, 4, 6)) and _same(a, b)
        n, d, s, M = 1000, 8, 0.1, 4100
        assert _beyond_direct(n, d, M) and not _beyond_direct(n, d, M - 4)
        x, y, h, w, s, xo, on = _case(n, d, s, M)
        a, b = (_both_routes(eng, x, y, h, w, s, xo, True) for eng in (engine, eng0))
    assert all(a[k] is not None for k in (0, 1, 2, 3, 4, 6)) and _same(a, b)
    mean, var, dmean, dvar, mean1, _, dmean1, _, pm, pv = a
    assert mean.shape == var.shape == (M,) and dmean.shape == dvar.shape == (d, M)
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)
    cols = np.r_[0:64, M - 64:M]
    assert on >= 64 and M - 64 >= on  # (the first 64 lie on training points, the last 64 off them)
    ref = _reference(oracle, x, y, h, w, s, np.asfortranarray(xo[:, cols]), 64)
    _check({"dmean": dmean[:, cols], "dvar": dvar[:, cols]}, *ref, ("dmean", "dvar"))
    _check({"mean": mean1[cols], "dmean": dmean1[:, cols]}, *ref, ("mean", "dmean"))


def test_leaves_the_fit_alone(engine):
    """predict, logml and alpha() read the same bits before and after a predict_grad.  And this
    consumer's own event test at its own shapes (the shared table of test_gp_fit_state.py holds
    it too, against every event and every other consumer): a warm fit that goes through refit,
    set_y + refit, append and remove, each after predict_grad calls on both routes -- so that
    every workspace and every piece of derived state is there to go stale -- gives the bits of a
    cold twin that goes through the same events and is asked only afterwards.  After the two
    refits, where the factor is a factorisation from nothing, those are also the bits of a
    fresh fit of the same data; an appended or shrunk factor is not a fresh factorisation bit
    for bit (predict differs there too), so there the twin is the only pin."""
    n, d, s, M = 130, 2, 0.1, 33
    x, y, h, w, s, xo, _ = _case(n, d, s, M)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        before = fit.predict(xo)[:2] + (fit.logml, fit.alpha())
        fit.predict_grad(xo)
        fit.predict_grad(xo, want_var=False)
        after = fit.predict(xo)[:2] + (fit.logml, fit.alpha())
        assert _same(before, after)
    finally:
        fit.close()

    def both(f):
        return f.predict_grad(xo), f.predict_grad(xo, want_var=False)

    def fresh(x, y, h, w, s):
        f = engine.gp_fit(x, y, h, w, s)
        try:
            return both(f)
        finally:
            f.close()

    def same2(a, b):
        return _same(a[0], b[0]) and _same(a[1], b[1])

    rs = np.random.RandomState(7)
    h2, w2, s2 = 1.1, w * 0.9, 0.2
    y2 = y + rs.randn(n)
    xa, ya = rs.uniform(-3, 3, size=(d, 3)), rs.randn(3)
    idx = np.array([2, 70, n + 1])
    events = [
        lambda f: f.refit(h2, w2, s2),
        lambda f: (f.set_y(y2), f.refit(h2, w2, s2)),
        lambda f: f.append(xa, ya),
        lambda f: f.remove(idx),
    ]
    from_nothing = {0: (x, y), 1: (x, y2)}
    warm = engine.gp_fit(x, y, h, w, s)
    try:
        both(warm)
        for k, event in enumerate(events):
            event(warm)
            got = both(warm)
            cold = engine.gp_fit(x, y, h, w, s)  # the same events, and asked only now
            try:
                for e in events[:k + 1]:
                    e(cold)
                assert warm.n == cold.n
                assert same2(got, both(cold)), "event %d" % k
            finally:
                cold.close()
            if k in from_nothing:
                assert same2(got, fresh(*from_nothing[k], h2, w2, s2)), "event %d" % k
        assert warm.n == n
    finally:
        warm.close()


def test_arguments(engine):
    from bayesian_quadrature_amd import _lib
    x, y, h, w, s, xo, _ = _case(65, 2, 0.1, 65)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        mean, var, dmean, dvar = fit.predict_grad(np.empty((2, 0)))
        assert mean.shape == var.shape == (0,) and dmean.shape == dvar.shape == (2, 0)
        mean, var, dmean, dvar = fit.predict_grad(np.empty((2, 0)), want_var=False)
        assert mean.shape == (0,) and dmean.shape == (2, 0) and var is None and dvar is None
        with pytest.raises(ValueError):
            fit.predict_grad(np.zeros((3, 4)))
        # all four outputs NULL through the raw ABI
        lib, dp = engine._lib, C.POINTER(C.c_double)
        st = lib.bq_gp_predict_grad(engine._ctx, fit._handle(), xo.ctypes.data_as(dp), 65, None,
                                    None, None, None)
        assert st == _lib.BQ_ERR_BAD_ARG == 2
        st = lib.bq_gp_predict_grad(engine._ctx, fit._handle(), None, 3, None, None,
                                    xo.ctypes.data_as(dp), None)
        assert st == 2
        # new targets and no refit: the error predict gives
        fit.set_y(y + 1.0)
        errs = []
        for call in (lambda: fit.predict(xo), lambda: fit.predict_grad(xo),
                     lambda: fit.predict_grad(xo, want_var=False)):
            with pytest.raises(Exception) as ei:
                call()
            errs.append((type(ei.value), str(ei.value)))
        assert errs[0] == errs[1] == errs[2] and "refit" in errs[0][1]
        fit.refit(h, w, s)
        assert fit.predict_grad(xo)[0].shape == (65,)
    finally:
        fit.close()
