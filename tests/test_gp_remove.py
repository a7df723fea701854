"""Removing observations from a resident GP fit (bq_gp_remove, engine.Fit.remove) on the device:
against the oracle's fresh fit of the surviving points at the bars of a grown fit
(test_gp_append._check_parity, imported: the same inputs, the same figures, the same bounds),
against fresh device fits bit for bit where the state must be the same, and at the engine's own
sizes."""
import contextlib

import numpy as np
import pytest

from bayesian_quadrature_amd import workloads as wl
from test_gp_append import (RTOL, _check_parity, _engine_env, _grad_T, _problem, _problem_d,
                            _same_bits, relmax)
from test_logml_hess import _reference as _hess_reference

pytestmark = pytest.mark.gpu


def _spread(n, k):
    """k distinct indices spread over [0, n), first and last included."""
    return np.unique(np.linspace(0, n - 1, k).round().astype(int))


def _removed(engine, x, y, h, w, s, idx, before=None):
    """A fit of all the points with idx removed (before: called on the fit first)."""
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        if before is not None:
            before(fit)
        fit.remove(idx)
    except Exception:
        fit.close()
        raise
    return fit


# ---- 1. parity ----------------------------------------------------------------------------
CASES_1D = [
    (8, [0]), (8, [7]), (64, [0]), (65, [64]), (65, [0]), (130, [3, 70, 129]),
    (130, [129, 3, 70]), (200, _spread(200, 64)), (200, _spread(200, 65)),
    (970, _spread(970, 12)), (1030, _spread(1030, 10)),
]


@pytest.mark.parametrize("n,idx", CASES_1D, ids=lambda v: str(v) if np.isscalar(v) else
                         "k%d_%d_%d" % (len(v), v[0], v[-1]))
def test_remove_parity_1d(engine, oracle, n, idx):
    idx = np.asarray(idx)
    assert np.unique(idx).size == idx.size
    x, y, h, w, s = _problem(n, seed=n)
    fit = _removed(engine, x, y, h, w, s, idx)
    try:
        _check_parity(engine, oracle, fit, np.delete(x, idx, axis=1), np.delete(y, idx), h, w, s,
                      tag="remove 1d (%d, %d)" % (n, idx.size))
    finally:
        fit.close()


@pytest.mark.parametrize("d", [2, 8])
def test_remove_parity_nd(engine, oracle, d):
    n, idx = 300, np.array([3, 77, 150, 222, 299])
    x, y, h, w, s = _problem_d(n, d, seed=n + 10 * d)
    assert np.linalg.cond(oracle.gram(x, h, w, s)) <= 1e7
    fit = _removed(engine, x, y, h, w, s, idx)
    try:
        _check_parity(engine, oracle, fit, np.delete(x, idx, axis=1), np.delete(y, idx), h, w, s,
                      tag="remove %dd" % d)
    finally:
        fit.close()


# ---- 2. a chain ---------------------------------------------------------------------------
def test_remove_chain_of_single_points(engine, oracle):
    """n = 200, then 130 single removals, first / middle / last in turn, down to 70: two 64-row
    boundaries (and two shrunk layouts)."""
    x, y, h, w, s = _problem(200, seed=200)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        worst = 0.0
        for step in range(130):
            n = x.shape[1]
            i = (0, n // 2, n - 1)[step % 3]
            fit.remove([i])
            x, y = np.delete(x, i, axis=1), np.delete(y, i)
            _, _, lmo = oracle.gp_fit(x, y, h, w, s)
            worst = max(worst, abs(fit.logml - lmo) / abs(lmo))
            assert fit.n == n - 1 and abs(fit.logml - lmo) <= RTOL * abs(lmo), step
        print("remove chain 200 - 130 x 1: worst log-ML error %.3g" % worst)
        _check_parity(engine, oracle, fit, x, y, h, w, s, tag="remove chain 200-130x1")
    finally:
        fit.close()


# ---- 3. the same state as a fresh fit -----------------------------------------------------
@pytest.mark.parametrize("n,idx", [(40, [5, 20, 39]), (100, _spread(100, 36)),
                                   (130, [0, 129]), (1030, _spread(1030, 10))],
                         ids=["40-3", "100-36", "130-2", "1030-10"])
def test_refit_after_remove_is_a_fresh_fit_bit_for_bit(engine, n, idx):
    """Points, targets, layout and workspaces after a remove are exactly a fresh fit's: a refit at
    new hyper-parameters gives the same bits as engine.gp_fit of the survivors there; so do
    set_y + refit and refit_predict."""
    idx = np.asarray(idx)
    x, y, h, w, s = _problem(n, seed=n)
    h2, w2, s2 = 0.9, 1.3 * w, 3e-2
    xo = np.linspace(-4, 4, 37)
    xs, ys = np.delete(x, idx, axis=1), np.delete(y, idx)

    def before(fit):  # workspaces and captured sweeps of the old size exist
        fit.predict(xo)
        fit.alpha()
        fit.logml_grad()

    fit = _removed(engine, x, y, h, w, s, idx, before)
    fresh = engine.gp_fit(xs, ys, h2, w2, s2)
    try:
        fit.refit(h2, w2, s2)
        _same_bits(fit, fresh, xo)
        y2 = np.cos(xs[0])
        fit.set_y(y2)
        fit.refit(h2, w2, s2)
        fresh.set_y(y2)
        fresh.refit(h2, w2, s2)
        _same_bits(fit, fresh, xo)
        xb = np.linspace(-3, 3, 20)
        ma, va = fit.refit_predict(h, w, s, xb)
        mb, vb = fresh.refit_predict(h, w, s, xb)
        assert np.array_equal(ma, mb) and np.array_equal(va, vb)
        _same_bits(fit, fresh, xo)
    finally:
        fit.close()
        fresh.close()


# ---- 4. remove after refit_predict --------------------------------------------------------
@pytest.mark.parametrize("n,idx", [(50, [0]), (200, _spread(200, 70))], ids=["50-1", "200-70"])
def test_remove_after_refit_predict(engine, oracle, n, idx):
    """refit_predict leaves border points in the layout and the y row behind them: the remove
    reads z from where it is."""
    idx = np.asarray(idx)
    x, y, h, w, s = _problem(n, seed=n + 7)
    fit = engine.gp_fit(x, y, 0.7, 2 * w, 0.1)
    try:
        fit.refit_predict(h, w, s, np.linspace(-4, 4, 33))
        fit.remove(idx)
        _check_parity(engine, oracle, fit, np.delete(x, idx, axis=1), np.delete(y, idx), h, w, s,
                      grad=False, tag="remove after refit_predict (%d, %d)" % (n, idx.size))
    finally:
        fit.close()


def test_trailing_remove_after_refit_predict(engine, oracle):
    x, y, h, w, s = _problem(50, seed=57)
    fit = engine.gp_fit(x, y, 0.7, 2 * w, 0.1)
    try:
        fit.refit_predict(h, w, s, np.linspace(-4, 4, 33))
        fit.remove([48, 49])
        _check_parity(engine, oracle, fit, x[:, :48], y[:48], h, w, s, grad=False,
                      tag="trailing remove after refit_predict")
    finally:
        fit.close()


# ---- 5. consumers straight after a remove -------------------------------------------------
@pytest.mark.parametrize("n,idx", [(100, [5, 50]), (130, [0, 129])], ids=["100-2", "130-2"])
def test_consumers_straight_after_a_remove(engine, oracle, n, idx):
    """No refit in between: predict (mean, var, cov), solve, alpha, the gradient and the Hessian
    against a fresh device fit of the survivors -- the values at RTOL, the gradient and the Hessian
    at their own tests' bars."""
    x, y, h, w, s = _problem_d(n, 2, seed=n)
    xs, ys = np.delete(x, idx, axis=1), np.delete(y, idx)
    rs = np.random.RandomState(n)
    xo = np.asfortranarray(rs.uniform(-3, 3, size=(2, 40)))
    b = rs.randn(n - len(idx), 3)

    def before(fit):
        fit.predict(xo)
        fit.logml_grad()
        fit.logml_hess()

    fit = _removed(engine, x, y, h, w, s, idx, before)
    fresh = engine.gp_fit(xs, ys, h, w, s)
    try:
        k0 = oracle.kernel_scale(2, h, w)
        for name, u, v, scale in zip(("mean", "var", "cov"), fit.predict(xo, want_cov=True),
                                     fresh.predict(xo, want_cov=True), (None, k0, k0)):
            assert relmax(u, v, scale) < RTOL, name
        assert relmax(fit.solve(b), fresh.solve(b)) < RTOL
        assert relmax(fit.alpha(), fresh.alpha()) < RTOL
        g, gf = fit.logml_grad(), fresh.logml_grad()
        T = _grad_T(oracle, xs, ys, h, w, s)
        print("remove (%d, %s) gradient: %s" % (n, idx, np.abs(g - gf) / T))
        assert np.all(np.abs(g - gf) <= 1e-8 * T), (g, gf, T)
        H, Hf = fit.logml_hess(), fresh.logml_hess()
        _, _, tol = _hess_reference(oracle, xs, ys, h, w, s)
        print("remove (%d, %s) Hessian: %s" % (n, idx, np.max(np.abs(H - Hf) / tol)))
        assert np.all(np.abs(H - Hf) <= tol), (H, Hf, tol)
    finally:
        fit.close()
        fresh.close()


# ---- 6. round trips -----------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(100, 10), (130, 3), (200, 70)])
def test_remove_the_last_then_append_them_back(engine, n, k):
    x, y, h, w, s = _problem(n, seed=n)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        L0, lm0 = fit.L(), fit.logml
        fit.remove(np.arange(n - k, n))
        assert np.array_equal(fit.L(), L0[:n - k, :n - k])  # no arithmetic on the factor
        fit.append(x[:, n - k:], y[n - k:])
        err = relmax(fit.L(), L0)
        print("remove last %d of %d, append: L %.3g" % (k, n, err))
        assert err < 1e-12 and abs(fit.logml - lm0) <= 1e-12 * abs(lm0)
    finally:
        fit.close()


def test_remove_a_spread_set_then_append_it(engine, oracle):
    n, idx = 200, _spread(200, 9)
    x, y, h, w, s = _problem(n, seed=n)
    fit = _removed(engine, x, y, h, w, s, idx)
    try:
        fit.append(x[:, idx], y[idx])
        xp = np.concatenate([np.delete(x, idx, axis=1), x[:, idx]], axis=1)
        yp = np.concatenate([np.delete(y, idx), y[idx]])
        _check_parity(engine, oracle, fit, xp, yp, h, w, s, tag="remove + append")
    finally:
        fit.close()


# ---- 7. determinism, block against single -------------------------------------------------
@pytest.mark.parametrize("n,idx", [(100, [7]), (200, _spread(200, 65)), (1030, _spread(1030, 10))],
                         ids=["100-1", "200-65", "1030-10"])
def test_remove_is_deterministic(engine, n, idx):
    x, y, h, w, s = _problem(n, seed=n)
    out = []
    for _ in range(2):
        fit = _removed(engine, x, y, h, w, s, idx)
        try:
            out.append((fit.logml, fit.L(), fit.z(), fit.alpha()))
        finally:
            fit.close()
    assert out[0][0] == out[1][0]
    for u, v in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("n,idx", [(100, _spread(100, 10)), (200, _spread(200, 70))],
                         ids=["100-10", "200-70"])
def test_remove_block_and_one_at_a_time_agree(engine, n, idx):
    x, y, h, w, s = _problem(n, seed=n)
    fa = _removed(engine, x, y, h, w, s, idx)
    fb = engine.gp_fit(x, y, h, w, s)
    try:
        for i in sorted(idx)[::-1]:
            fb.remove([i])
        err = relmax(fa.L(), fb.L())
        print("remove (%d, %d) block against one at a time: %.3g" % (n, len(idx), err))
        assert err < 1e-12
        assert abs(fa.logml - fb.logml) <= 1e-12 * abs(fb.logml)
    finally:
        fa.close()
        fb.close()


# ---- 8. status rules ----------------------------------------------------------------------
def test_remove_argument_errors(engine):
    x, y, h, w, s = _problem(50, seed=50)
    fit = engine.gp_fit(x, y, h, w, s)

    def state():
        return fit.n, fit.logml, fit.L(), fit.alpha()

    before = state()
    for idx in (None, [], np.arange(50), np.arange(51), [50], [-1], [3, 3], [3, 7, 3], [1.0],
                [[1, 2]]):
        with pytest.raises(ValueError):
            fit.remove(idx)
        after = state()
        assert before[0] == after[0] == 50 and before[1] == after[1], idx
        assert np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3]), idx
    fit.set_y(np.cos(x[0]))
    with pytest.raises(ValueError):        # stale: refit required, as every consumer says
        fit.remove([3])
    assert fit.n == 50
    fit.refit(h, w, s)
    fit.remove([3])
    assert fit.n == 49
    fit.close()
    with pytest.raises(ValueError):
        fit.remove([3])


# ---- 9. scale -----------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"BQ_GRAPH": "0"}], ids=["default", "BQ_GRAPH=0"])
@pytest.mark.parametrize("N,k", [(4096 + 64, 64), (16384, 1)])
def test_remove_at_scale(engine, env, N, k):
    """workloads.c4's inputs with the middle indices removed; no oracle factor at this size: the
    survivors' rows of L from the first removed index on and log-ML against a fresh device fit,
    and 200 sampled entries of L L^T against the closed-form kernel.  An entry of the computed
    factor's L L^T is within (N + 1) eps sqrt(K_ii K_jj) of K_ij (Higham, Accuracy and Stability,
    thm 10.3 and (10.7))."""
    c = wl.c4(N)
    xs, h, w, s = c["x"], c["h"], c["w"], c["s"]
    ys = wl.norm_logpdf(xs)
    first = N // 2 - k // 2 - (k == 1)     # (16384, [8191])
    idx = np.arange(first, first + k)
    x, y = np.delete(xs, idx), np.delete(ys, idx)
    n = N - k
    with (_engine_env(env) if env else contextlib.nullcontext(engine)) as eng:
        fresh = eng.gp_fit(x, y, h, w, s)
        lm_fresh = fresh.logml
        rows_fresh = fresh.L()[first:].copy()
        fresh.close()
        fit = eng.gp_fit(xs, ys, h, w, s)
        try:
            fit.remove(idx)
            lm = fit.logml
            L = fit.L()
        finally:
            fit.close()
    assert L.shape == (n, n)
    e_rows = relmax(L[first:], rows_fresh)
    e_lm = abs(lm - lm_fresh) / abs(lm_fresh)
    print("remove at scale (%d, %d) %s: rows %.3g log-ML %.3g" % (N, k, env, e_rows, e_lm))
    assert e_rows < RTOL and e_lm <= RTOL
    rs = np.random.RandomState(N)
    ii = np.concatenate([rs.randint(first, n, 120), rs.randint(0, n, 80)])
    jj = np.clip(ii + rs.randint(-6, 7, 200), 0, n - 1)  # neighbours in x: entries that are not 0
    k0 = h * h / (np.sqrt(2 * np.pi) * w[0])
    worst = 0.0
    for i, j in zip(ii, jj):
        got = float(np.dot(L[i], L[j]))
        want = k0 * np.exp(-0.5 * ((x[i] - x[j]) / w[0]) ** 2) + (s * s if i == j else 0.0)
        worst = max(worst, abs(got - want) / (k0 + s * s))
    print("remove at scale (%d, %d): worst sampled |LL^T - K| / K_ii %.3g" % (N, k, worst))
    assert worst <= (N + 1) * np.finfo(np.float64).eps
