"""Derivatives of the posterior mean and variance in the hyper-parameters on the device
(bq_gp_predict_dtheta, engine.Fit.predict_dtheta: both routes) against explicit CPU references.

The method of test_predict_grad.py.  The tolerances are measured, not fixed: the reference comes
from Kxx^-1, a, u, z_k, beta, q_jk and every sum at 50 digits (n <= 65) or from the oracle's
factor and numpy; a second float64 route with the device's own algebra (Cholesky, the explicit
Y = L^-T, beta = K(xo, x) Y Y^T, the solves through Y) gives, per quantity,
r = max |cpu - ref| / T, and the device gets 100 max(r, 4 eps) T.  T is the norm-product size of
an entry's terms (test_predict_dtheta_host.term_sizes), not the sum of |term|: at a query on a
training point with s = 0, beta_j is a unit vector and the term sum collapses to rounding noise.
The first min(M // 4, n) queries are training points exactly.

The bound cannot hide a wrong entry: tol <= 1e-2 |ref| is asserted for every entry but those whose
true value is zero or cancels by construction -- the h row of dmean and the s rows of both at
s = 0 (exactly 0.0 on the device: T = 0 there), dvar at the queries on training points, and at
s = 0 also the w rows of dmean at those queries: without noise the mean there is y_i whatever the
length scales, so sum_i k_ji g_jik a_i and sum_i k_ji z_k,i cancel to rounding."""
import ctypes as C
import functools

import numpy as np
import pytest

from engine_env import engine_env
from test_predict_dtheta_host import _dk, closed_form, numpy_pieces, term_sizes

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0
NAMES = ("mean", "dmean", "dvar")


def _case(n, d, s, M):
    rs = np.random.RandomState(n + 10 * d)
    x = rs.uniform(-3.0, 3.0, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    w = rs.uniform(0.6, 1.2, size=d)
    if s < 1e-2 or d == 8:  # points well apart: Kxx stays well conditioned with little noise
        w = w * 0.25
    xo = np.random.RandomState(1000 + n).uniform(-3.3, 3.3, size=(d, M))
    on = min(M // 4, n)
    xo[:, :on] = x[:, :on]
    return x, y, 1.3, w, float(s), np.asfortranarray(xo), on


def _mp_reference(x, y, h, w, s, xo):
    """(pieces, mean, dmean, dvar): Kxx^-1, a, u, z_k, beta, q_jk and every sum at 50 digits (the
    construction of test_logml_hess._mp_inverse), rounded only at the end; pieces: the operands of
    term_sizes as float64 arrays."""
    import mpmath as mp
    mp.mp.dps = 50
    d, n = x.shape
    M = xo.shape[1]
    X = [[mp.mpf(float(x[k, i])) for i in range(n)] for k in range(d)]
    XO = [[mp.mpf(float(xo[k, j])) for j in range(M)] for k in range(d)]
    W = [mp.mpf(float(w[k])) for k in range(d)]
    H, S = mp.mpf(h), mp.mpf(s)
    c = H ** 2
    for k in range(d):
        c /= mp.sqrt(2 * mp.pi) * W[k]

    def kern(p, q):
        return c * mp.exp(-sum((p[k] - q[k]) ** 2 / (2 * W[k] ** 2) for k in range(d)))

    K0 = mp.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):
            K0[i, j] = K0[j, i] = kern([X[k][i] for k in range(d)], [X[k][j] for k in range(d)])
    Kxx = K0.copy()
    for i in range(n):
        Kxx[i, i] += S ** 2
    Ki = Kxx ** -1
    a = Ki * mp.matrix([mp.mpf(float(v)) for v in y])
    u = Ki * a
    D = []
    for k in range(d):
        Dk = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                Dk[i, j] = K0[i, j] * ((X[k][i] - X[k][j]) ** 2 / W[k] ** 3 - 1 / W[k])
        D.append(Dk)
    z = [Ki * (D[k] * a) for k in range(d)]
    K = mp.matrix(M, n)
    for j in range(M):
        for i in range(n):
            K[j, i] = kern([XO[k][j] for k in range(d)], [X[k][i] for k in range(d)])
    B = K * Ki  # row j = (Kxx^-1 k_j)^T
    BD = [B * D[k] for k in range(d)]
    mean = np.empty(M)
    dmean, dvar = np.empty((d + 2, M)), np.empty((d + 2, M))
    for j in range(M):
        mean[j] = float(sum(K[j, i] * a[i] for i in range(n)))
        ku = sum(K[j, i] * u[i] for i in range(n))
        bb = sum(B[j, i] ** 2 for i in range(n))
        var = c - sum(K[j, i] * B[j, i] for i in range(n))
        dmean[0, j] = float(2 * S ** 2 / H * ku)
        dmean[d + 1, j] = float(-2 * S * ku)
        dvar[0, j] = float(2 / H * (var - S ** 2 * bb))
        dvar[d + 1, j] = float(2 * S * bb)
        for k in range(d):
            g = [(XO[k][j] - X[k][i]) ** 2 / W[k] ** 3 - 1 / W[k] for i in range(n)]
            dmean[1 + k, j] = float(sum(K[j, i] * (g[i] * a[i] - z[k][i]) for i in range(n)))
            q = sum(BD[k][j, i] * B[j, i] for i in range(n))
            dvar[1 + k, j] = float(-c / W[k] - 2 * sum(K[j, i] * g[i] * B[j, i] for i in range(n))
                                   + q)

    def arr(m_, r, c_):
        return np.array([[float(m_[i, j]) for j in range(c_)] for i in range(r)])

    def vec(v):
        return np.array([float(v[i]) for i in range(n)])

    pieces = dict(k0=float(c), K=arr(K, M, n), K0=arr(K0, n, n), a=vec(a), u=vec(u),
                  z=np.array([vec(z[k]) for k in range(d)]), beta=arr(B, M, n))
    return pieces, mean, dmean, dvar


def _device_algebra(oracle, x, y, h, w, s, xo):
    """The device's own route in float64 on the CPU: {"mean", "dmean", "dvar"}."""
    from scipy.linalg import solve_triangular
    d, n = x.shape
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    Y = solve_triangular(Lc, np.eye(n), lower=True).T

    def solve(v):
        return Y @ (Y.T @ v)

    K = np.ascontiguousarray(oracle.gram_cross(xo, x, h, w))
    K0 = np.ascontiguousarray(oracle.gram(x, h, w, 0.0))
    k0 = oracle.kernel_scale(d, h, w)
    V = K @ Y
    a = solve(y)
    p = dict(k0=k0, K=K, K0=K0, a=a, u=solve(a),
             z=np.array([solve(_dk(x, K0, w, k) @ a) for k in range(d)]), beta=V @ Y.T,
             var=k0 - np.sum(V * V, axis=1))
    dmean, dvar = closed_form(x, xo, h, w, s, **p)
    return {"mean": K @ a, "dmean": dmean, "dvar": dvar}


def _reference(oracle, x, y, h, w, s, xo, on):
    """(ref, T, tol), each a dict over NAMES; prints r per quantity."""
    d, n = x.shape
    M = xo.shape[1]
    if n <= 65:
        p, mean, dmean, dvar = _mp_reference(x, y, h, w, s, xo)
    else:
        p = numpy_pieces(oracle, x, y, h, w, s, xo)
        dmean, dvar = closed_form(x, xo, h, w, s, **p)
        mean = p["K"] @ p["a"]
        p.pop("var")
    ref = {"mean": mean, "dmean": dmean, "dvar": dvar}
    Tm, Tv = term_sizes(x, xo, h, w, s, **p)
    T = {"mean": np.abs(p["K"]) @ np.abs(p["a"]), "dmean": Tm, "dvar": Tv}
    cpu = _device_algebra(oracle, x, y, h, w, s, xo)
    tol = {}
    for q in NAMES:
        pos = T[q] > 0
        r = float(np.max((np.abs(cpu[q] - ref[q])[pos]) / T[q][pos])) if pos.any() else 0.0
        tol[q] = MARGIN * max(r, 4 * EPS) * T[q]
        print("n=%d d=%d s=%g M=%d %s: r %.3g" % (n, d, s, M, q, r))
    # the bound cannot hide a wrong entry, but for the entries the module's docstring names
    held_m = np.ones((d + 2, M), dtype=bool)
    held_v = np.ones((d + 2, M), dtype=bool)
    held_v[:, :on] = False
    if s == 0.0:
        held_m[[0, d + 1]] = False
        held_m[:, :on] = False  # (the posterior interpolates y there whatever the length scales)
        held_v[d + 1] = False
        assert np.all(Tm[[0, d + 1]] == 0.0) and np.all(Tv[d + 1] == 0.0)
        assert np.all(dmean[[0, d + 1]] == 0.0) and np.all(dvar[d + 1] == 0.0)
    assert np.all(tol["dmean"][held_m] <= 1e-2 * np.abs(dmean[held_m])), \
        (tol["dmean"], dmean)
    assert np.all(tol["dvar"][held_v] <= 1e-2 * np.abs(dvar[held_v])), (tol["dvar"], dvar)
    return ref, T, tol


# (n, d, s, M): npad 64 / 128 / 192 / 320, n below, on and past a 64 boundary and no multiple of
# the quad product's 16-column chunk, M on both sides of the 16-row workgroup and the 64-row
# padding (Mp 64 / 128 / 320: one to five row tiles of the 64 x 64 quad tile), d = 8 (the widest
# template), s = 0
CASES = [
    (1, 1, 0.1, 1), (9, 2, 0.0, 17), (63, 1, 0.1, 64), (64, 8, 1e-3, 15), (65, 2, 0.1, 65),
    (130, 3, 0.1, 16), (300, 3, 0.0, 63), (300, 1, 0.1, 300),
]
# the quad product's second row tile, 256 x 64 (BQ_GEMM_TILE=128 selects it where the rule would
# not): Mp = 64, a tile three quarters beyond the last row, and Mp = 320, a second tile that is
TALL_CASES = [(300, 3, 0.0, 63), (300, 1, 0.1, 300)]


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
        mean, var, dmean, dvar = fit.predict_dtheta(xo)
        pm, pv, _ = fit.predict(xo)
    finally:
        fit.close()
    assert mean.shape == var.shape == (M,) and dmean.shape == dvar.shape == (d + 2, M)
    _check({"dmean": dmean, "dvar": dvar}, *_case_reference(oracle, n, d, s, M),
           ("dmean", "dvar"))
    # the sweep and the row reductions are bq_gp_predict's own
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)


def _mean_route(engine, oracle, n, d, s, M):
    x, y, h, w, s, xo, on = _case(n, d, s, M)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        mean, var, dmean, dvar = fit.predict_dtheta(xo, want_var=False)
    finally:
        fit.close()
    assert var is None and dvar is None
    assert mean.shape == (M,) and dmean.shape == (d + 2, M)
    _check({"mean": mean, "dmean": dmean}, *_case_reference(oracle, n, d, s, M),
           ("mean", "dmean"))


@pytest.mark.parametrize("n,d,s,M", CASES)
def test_full_route_against_reference(engine, oracle, n, d, s, M):
    _full(engine, oracle, n, d, s, M)


@pytest.mark.parametrize("n,d,s,M", CASES)
def test_mean_route_against_reference(engine, oracle, n, d, s, M):
    _mean_route(engine, oracle, n, d, s, M)


@pytest.mark.parametrize("n,d,s,M", TALL_CASES)
def test_tall_row_tile_against_reference(oracle, n, d, s, M):
    with engine_env({"BQ_GEMM_TILE": "128"}) as eng:
        _full(eng, oracle, n, d, s, M)


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
            a, b = fit.predict_dtheta(xo), fit.predict_dtheta(xo)
            assert all(v is not None for v in a) and _same(a, b)
            a, b = fit.predict_dtheta(xo, want_var=False), fit.predict_dtheta(xo, want_var=False)
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
        out = fit.predict_dtheta(xo) + fit.predict_dtheta(xo, want_var=False)
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
    assert mean.shape == var.shape == (M,) and dmean.shape == dvar.shape == (d + 2, M)
    assert np.array_equal(mean, pm) and np.array_equal(var, pv)
    cols = np.r_[0:64, M - 64:M]
    assert on >= 64 and M - 64 >= on  # (the first 64 lie on training points, the last 64 off them)
    ref = _reference(oracle, x, y, h, w, s, np.asfortranarray(xo[:, cols]), 64)
    _check({"dmean": dmean[:, cols], "dvar": dvar[:, cols]}, *ref, ("dmean", "dvar"))
    _check({"mean": mean1[cols], "dmean": dmean1[:, cols]}, *ref, ("mean", "dmean"))


def test_leaves_the_fit_alone(engine):
    """predict, logml, alpha(), logml_hess() and predict_grad read the same bits before and after
    a predict_dtheta.  And the DKZ bit's own event test at its own shapes (the shared table of
    test_gp_fit_state.py holds it too, against every event and every other consumer): a warm fit
    that goes through refit, set_y + refit, append and remove, each after predict_dtheta calls on both
    routes -- so that the solved vectors, every workspace and every piece of derived state are
    there to go stale -- gives the bits of a cold twin that goes through the same events and is
    asked only afterwards.  After the two refits, where the factor is a factorisation from
    nothing, those are also the bits of a fresh fit of the same data."""
    n, d, s, M = 130, 2, 0.1, 33
    x, y, h, w, s, xo, _ = _case(n, d, s, M)

    def state(f):
        return (f.predict(xo)[:2] + (f.logml, f.alpha(), f.logml_hess()) + f.predict_grad(xo)
                + f.predict_grad(xo, want_var=False))

    fit = engine.gp_fit(x, y, h, w, s)
    try:
        before = state(fit)
        fit.predict_dtheta(xo)
        fit.predict_dtheta(xo, want_var=False)
        assert _same(before, state(fit))
    finally:
        fit.close()

    def both(f):
        return f.predict_dtheta(xo), f.predict_dtheta(xo, want_var=False)

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
        last = both(warm)
        for k, event in enumerate(events):
            event(warm)
            got = both(warm)
            assert not same2(got, last), "event %d changed nothing" % k
            last = got
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
        mean, var, dmean, dvar = fit.predict_dtheta(np.empty((2, 0)))
        assert mean.shape == var.shape == (0,) and dmean.shape == dvar.shape == (4, 0)
        mean, var, dmean, dvar = fit.predict_dtheta(np.empty((2, 0)), want_var=False)
        assert mean.shape == (0,) and dmean.shape == (4, 0) and var is None and dvar is None
        with pytest.raises(ValueError):
            fit.predict_dtheta(np.zeros((3, 4)))
        # all four outputs NULL through the raw ABI
        lib, dp = engine._lib, C.POINTER(C.c_double)
        st = lib.bq_gp_predict_dtheta(engine._ctx, fit._handle(), xo.ctypes.data_as(dp), 65, None,
                                      None, None, None)
        assert st == _lib.BQ_ERR_BAD_ARG == 2
        st = lib.bq_gp_predict_dtheta(engine._ctx, fit._handle(), None, 3, None, None,
                                      xo.ctypes.data_as(dp), None)
        assert st == 2
        # any single output alone, through the raw ABI, is what the full call gives
        full = fit.predict_dtheta(xo)
        for k, shape in enumerate(((65,), (65,), (4, 65), (4, 65))):
            out = np.empty(shape, order="F")
            ptrs = [None] * 4
            ptrs[k] = out.ctypes.data_as(dp)
            st = lib.bq_gp_predict_dtheta(engine._ctx, fit._handle(), xo.ctypes.data_as(dp), 65,
                                          *ptrs)
            assert st == 0
            if k in (1, 3):  # (the mean and dmean alone take the route without a sweep)
                assert np.array_equal(out, full[k]), k
        # new targets and no refit: the error predict gives
        fit.set_y(y + 1.0)
        errs = []
        for call in (lambda: fit.predict(xo), lambda: fit.predict_dtheta(xo),
                     lambda: fit.predict_dtheta(xo, want_var=False)):
            with pytest.raises(Exception) as ei:
                call()
            errs.append((type(ei.value), str(ei.value)))
        assert errs[0] == errs[1] == errs[2] and "refit" in errs[0][1]
        fit.refit(h, w, s)
        assert fit.predict_dtheta(xo)[0].shape == (65,)
    finally:
        fit.close()
