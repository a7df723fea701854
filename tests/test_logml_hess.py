"""The analytic Hessian of the GP log marginal likelihood on the device (bq_gp_logml_hess,
engine.Fit.logml_hess, gp.GP.d2loglh_dtheta2, gp.GP.hyper_cov) against explicit CPU references.

The tolerance is measured, not fixed: a second float64 route with the device's own algebra
(Cholesky, Y = L^-T, Kxx^-1 = Y Y^T) gives r = max |H_cpu - H_ref| / T against the reference, T
being the size of each entry's terms; the device gets 100 max(r, 4 eps) T."""
import functools

import numpy as np
import pytest

from bayesian_quadrature_amd import gp as gp_mod

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0


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


def _derivatives(x, h, w, s, K0):
    """(D_p, D_pq) of Kxx over [h, w_1 .. w_d, s]; D_pq[p][q] is None where it vanishes."""
    d, n = x.shape
    r2 = [(x[k][:, None] - x[k][None, :]) ** 2 for k in range(d)]
    u = [r2[k] / w[k] ** 3 - 1.0 / w[k] for k in range(d)]
    D1 = [2.0 * K0 / h] + [K0 * u[k] for k in range(d)] + [2.0 * s * np.eye(n)]
    P = d + 2
    D2 = [[None] * P for _ in range(P)]
    D2[0][0] = 2.0 * K0 / h ** 2
    for k in range(d):
        D2[0][1 + k] = D2[1 + k][0] = 2.0 * D1[1 + k] / h
        for l in range(d):
            D2[1 + k][1 + l] = K0 * (u[k] * u[l] + (k == l) * (1.0 / w[k] ** 2
                                                               - 3.0 * r2[k] / w[k] ** 4))
    D2[P - 1][P - 1] = 2.0 * np.eye(n)
    return D1, D2


def _hessian(Ki, a, s, D1, D2, want_T=False):
    """H_pq = 1/2 sum(G o D_pq) - (D_p a)^T Ki (D_q a) + 1/2 tr(Ki D_p Ki D_q), and the size of
    its terms T_pq = 1/2 sum((|a a^T| + |Ki|) o |D_pq|) + |D_p a|^T |Ki| |D_q a|
    + 1/2 sum(|B_p| o |B_q^T|) with B_p = Ki D_p computed as it is."""
    P = len(D1)
    aa = np.outer(a, a)
    G = aa - Ki
    B = [Ki @ D for D in D1[:-1]] + [2.0 * s * Ki]  # (D_s = 2 s I)
    v = [D @ a for D in D1]
    H, T = np.zeros((P, P)), np.zeros((P, P))
    if want_T:
        A, aKi = np.abs(aa) + np.abs(Ki), np.abs(Ki)
        aB, av = [np.abs(b) for b in B], [np.abs(t) for t in v]
    for p in range(P):
        for q in range(p, P):
            t1 = 0.0 if D2[p][q] is None else 0.5 * np.sum(G * D2[p][q])
            H[p, q] = H[q, p] = t1 - v[p] @ (Ki @ v[q]) + 0.5 * np.sum(B[p] * B[q].T)
            if want_T:
                t1 = 0.0 if D2[p][q] is None else 0.5 * np.sum(A * np.abs(D2[p][q]))
                T[p, q] = T[q, p] = t1 + av[p] @ (aKi @ av[q]) + 0.5 * np.sum(aB[p] * aB[q].T)
    return H, T


def _mp_inverse(x, y, h, w, s):
    """(Kxx^-1, Kxx^-1 y) at 50 digits, rounded to float64."""
    import mpmath as mp
    mp.mp.dps = 50
    d, n = x.shape
    c = mp.mpf(h) ** 2
    for k in range(d):
        c /= mp.sqrt(2 * mp.pi) * mp.mpf(float(w[k]))
    K = mp.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):
            q = mp.mpf(0)
            for k in range(d):
                q += (mp.mpf(float(x[k, i])) - mp.mpf(float(x[k, j]))) ** 2 / (2 * mp.mpf(float(w[k])) ** 2)
            K[i, j] = K[j, i] = c * mp.exp(-q)
        K[i, i] += mp.mpf(s) ** 2
    Ki = K ** -1
    a = Ki * mp.matrix([mp.mpf(float(v)) for v in y])
    return (np.array([[float(Ki[i, j]) for j in range(n)] for i in range(n)]),
            np.array([float(a[i]) for i in range(n)]))


def _reference(oracle, x, y, h, w, s):
    """(H_ref, T, tol): the reference Hessian, the size of its entries' terms and the entrywise
    bound 100 max(r, 4 eps) T with r measured on a second float64 route."""
    from scipy.linalg import solve_triangular
    d, n = x.shape
    K0 = oracle.gram(x, h, w, 0.0)
    D1, D2 = _derivatives(x, h, w, s, K0)
    if n <= 65:
        Ki, a = _mp_inverse(x, y, h, w, s)
    else:
        L, a, _ = oracle.gp_fit(x, y, h, w, s)
        Ki = oracle.cho_solve(L, np.eye(n))
    H_ref, T = _hessian(Ki, a, s, D1, D2, want_T=True)
    # the device's own algebra in float64 on the CPU
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    Y = solve_triangular(Lc, np.eye(n), lower=True).T
    a2 = solve_triangular(Lc, solve_triangular(Lc, y, lower=True), lower=True, trans="T")
    H_cpu, _ = _hessian(Y @ Y.T, a2, s, D1, D2)
    pos = T > 0
    r = float(np.max(np.abs(H_cpu - H_ref)[pos] / T[pos]))
    tol = MARGIN * max(r, 4 * EPS) * T
    print("n=%d d=%d s=%g: cond %.3g r %.3g" % (n, d, s, np.linalg.cond(K0 + s * s * np.eye(n)), r))
    # the bound cannot hide a wrong diagonal entry
    dg = np.arange(d + 2)
    assert np.all(tol[dg, dg] <= 1e-2 * np.abs(H_ref[dg, dg])), (tol[dg, dg], H_ref[dg, dg])
    return H_ref, T, tol


# (n, d, s): npad 64 / 128 / 320 / 1024 / 1152 / 2048, n on both sides of a 64 boundary, d = 8
# (the widest template) and s = 0
CASES = [
    (1, 1, 0.1), (9, 2, 0.0), (63, 1, 0.1), (64, 8, 1e-3), (65, 2, 0.1), (300, 3, 0.1),
    (1000, 1, 0.1), (1100, 3, 0.1), (2048, 1, 0.1),
]


@functools.lru_cache(maxsize=None)
def _case_reference(oracle, n, d, s):
    return _reference(oracle, *_case(n, d, s))


def _check(H, H_ref, T, tol):
    err = np.abs(H - H_ref)
    print("worst |H_dev - H_ref| / tol: %.3g" % float(np.max(err[T > 0] / tol[T > 0])))
    assert np.all(err <= tol), (H, H_ref, tol)
    assert np.all(H[T == 0] == 0.0), (H, T)


@pytest.mark.parametrize("n,d,s", CASES)
def test_logml_hess_matches_cpu_reference(engine, oracle, n, d, s):
    x, y, h, w, s = _case(n, d, s)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        H = fit.logml_hess()
    finally:
        fit.close()
    assert H.shape == (d + 2, d + 2)
    _check(H, *_case_reference(oracle, n, d, s))


@pytest.mark.parametrize("n,d,s", CASES)
def test_logml_hess_scaling_identity(engine, oracle, n, d, s):
    """h^2 H_hh + 2 h s H_hs + s^2 H_ss = n - 3 y^T a: exact, no reference needed."""
    x, y, h, w, s = _case(n, d, s)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        H = fit.logml_hess()
        a = fit.alpha()
    finally:
        fit.close()
    _, T, tol = _case_reference(oracle, n, d, s)
    lhs = h * h * H[0, 0] + 2 * h * s * H[0, d + 1] + s * s * H[d + 1, d + 1]
    bound = h * h * tol[0, 0] + 2 * h * s * tol[0, d + 1] + s * s * tol[d + 1, d + 1]
    print("identity: %.3g of its bound" % (abs(lhs - (n - 3 * float(y @ a))) / bound))
    assert abs(lhs - (n - 3 * float(y @ a))) <= bound, (lhs, n - 3 * float(y @ a), bound)


@pytest.mark.parametrize("n,d,s", [(300, 3, 0.1), (1100, 3, 0.1)])
def test_logml_hess_tall_tile(engine, oracle, n, d, s, monkeypatch):
    """The 256 x 64 workgroup tile of the products, which the large systems take, forced on
    systems whose npad (320, 1152) is no multiple of its 256 rows."""
    from bayesian_quadrature_amd.engine import Engine
    x, y, h, w, s = _case(n, d, s)
    monkeypatch.setenv("BQ_GEMM_TILE", "128")
    eng = Engine(0)
    try:
        fit = eng.gp_fit(x, y, h, w, s)
        try:
            H = fit.logml_hess()
        finally:
            fit.close()
    finally:
        eng.close()
    _check(H, *_case_reference(oracle, n, d, s))


def test_logml_hess_is_symmetric_deterministic_and_isolated(engine, oracle):
    x, y, h, w, s = _problem(1000, 2, 0.1, seed=5)
    xo = np.random.RandomState(6).uniform(-3, 3, size=(2, 50))
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        lm0, a0 = fit.logml, fit.alpha()
        m0, v0, _ = fit.predict(xo)
        g0 = fit.logml_grad()
        H1 = fit.logml_hess()
        H2 = fit.logml_hess()
        assert np.array_equal(H1, H1.T)
        assert np.array_equal(H1, H2)
        assert fit.logml == lm0
        assert np.array_equal(fit.alpha(), a0)
        m1, v1, _ = fit.predict(xo)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
        assert np.array_equal(fit.logml_grad(), g0)
        # after a refit: the Hessian of a fresh fit at the same parameters, same bits
        w2 = w * 1.3
        fit.refit(h * 0.9, w2, 0.05)
        H3 = fit.logml_hess()
        fresh = engine.gp_fit(x, y, h * 0.9, w2, 0.05)
        try:
            assert np.array_equal(H3, fresh.logml_hess())
        finally:
            fresh.close()
        assert not np.array_equal(H1, H3)
        # after an append: the Hessian of a fresh fit on the concatenated data, within the bound
        rs = np.random.RandomState(7)
        xn = rs.uniform(-3, 3, size=(2, 3))
        yn = np.sin(xn).sum(axis=0) + 0.1 * rs.randn(3)
        fit.refit(h, w, s)
        fit.logml_hess()
        fit.append(xn, yn)
        H4 = fit.logml_hess()
        xa, ya = np.concatenate([x, xn], axis=1), np.concatenate([y, yn])
        fresh = engine.gp_fit(xa, ya, h, w, s)
        try:
            H5 = fresh.logml_hess()
        finally:
            fresh.close()
        assert H4.shape == H5.shape and not np.array_equal(H4, H1)
        _, T, tol = _reference(oracle, xa, ya, h, w, s)
        assert np.all(np.abs(H4 - H5) <= tol), (H4, H5, tol)
    finally:
        fit.close()


def test_logml_hess_status_rules(engine):
    x, y, h, w, s = _problem(100, 1, 0.1, seed=7)
    xd = np.concatenate([x, x], axis=1)
    yd = np.concatenate([y, y])
    fit = engine.gp_fit(xd, yd, h, w, s)
    try:
        with pytest.raises(np.linalg.LinAlgError):
            fit.refit(h, w, 0.0)  # repeated points without noise
        with pytest.raises(np.linalg.LinAlgError):
            fit.logml_hess()
        fit.refit(h, w, s)
        fit.logml_hess()
        fit.set_y(yd + 1.0)
        with pytest.raises(ValueError):
            fit.logml_hess()
    finally:
        fit.close()
    with pytest.raises(ValueError):
        fit.logml_hess()


def test_gp_d2loglh_dtheta2(engine):
    x, y, h, w, s = _problem(500, 1, 0.1, seed=8)
    g = gp_mod.GP(gp_mod.GaussianKernel(h, w[0]), x[0], y, s=s)
    H1 = g.d2loglh_dtheta2
    assert H1.shape == (3, 3)
    assert H1 is g.d2loglh_dtheta2
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        assert np.array_equal(H1, fit.logml_hess())
    finally:
        fit.close()
    g.set_param("w", w[0] * 1.1)
    H2 = g.d2loglh_dtheta2
    assert H2 is not H1 and not np.array_equal(H1, H2)
    g.y = y + 0.5
    H3 = g.d2loglh_dtheta2
    assert H3 is not H2 and not np.array_equal(H2, H3)


def test_gp_hyper_cov_after_fit_MLII(engine, oracle):
    rs = np.random.RandomState(11)
    n = 1024
    x = np.sort(rs.uniform(-5, 5, size=n))
    h0, w0, s0 = 1.0, 0.7, 0.1
    K = oracle.gram(x[None, :], h0, np.array([w0]), s0)
    y = np.linalg.cholesky(K) @ rs.randn(n)
    g = gp_mod.GP(gp_mod.GaussianKernel(1.7 * h0, 0.6 * w0), x, y, s=2 * s0)
    assert g.fit_MLII(["h", "w", "s"]).success
    C = g.hyper_cov(["h", "w", "s"])
    assert C.shape == (3, 3) and np.array_equal(C, C.T)
    assert np.all(np.linalg.eigvalsh(C) > 0)
    H = g.d2loglh_dtheta2
    assert g.hyper_cov(["w"]).shape == (1, 1)
    assert g.hyper_cov(["w"])[0, 0] == -1.0 / H[1, 1]
