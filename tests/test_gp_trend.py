"""The polynomial trend of a resident fit on the device (bq_gp_trend, bq_gp_predict_trend,
engine.Fit.trend / predict_trend) against the long-double restatement of test_gp_trend_host.py.

Problems are test_gp_sample.py's ``_case(n, d, s, M, 1.0)`` with the Python surface's default
centre and scale.  The tolerance is measured, as in test_gp_ivr.py: the float64 restatement
(``numpy_trend``) runs on the oracle's Gram, Cholesky and triangular solves, its largest error
against long double relative to a scale is r, and the device gets 100 max(r, 4 eps) times the scale:
  mean      max_j (|v_j| |z| + sum_k |r_jk| |beta_k|)
  variance  k0 + max |v_j|^2 + max r_j^T A^-1 r_j
  beta_k    (|A^-1| |b|)_k
  logml_t   (|z|^2 + |b^T beta|) / 2 + |log det Kxx| + |log det A|
and, by the same rule, cov_beta relative to max |A^-1|, alpha_t to max |alpha_t| and (H^T alpha_t)_k
-- exactly 0 -- to (|H|^T |alpha_t|)_k.  Before the device is looked at the reference alone must
show cond(A) <= 1e3 and a largest r^T A^-1 r of at least 1e-4 of the variance scale: a device that
dropped the correction cannot pass."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gp_sample import _case
from test_gp_trend_host import (LD, default_basis, ld_trend, numpy_trend, scales, trend_basis,
                                trend_p)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0

# (n, d, s, M, degree): p = 1 with npad = 128, one row in the second block, M past one 64-block;
# p = 3; p = 4; p = 6; the row reductions' 8-wide trip (npad = 256); p = 10, the product route;
# p = 9, the first size past the one-pass route; p = 45; one query point
CASES = [
    (65, 1, 0.1, 70, 0),
    (65, 1, 0.1, 70, 2),
    (65, 3, 0.1, 64, 1),
    (130, 2, 0.05, 130, 2),
    (200, 3, 0.1, 70, 1),
    (130, 3, 0.1, 100, 2),
    (130, 8, 0.1, 40, 1),
    (130, 8, 0.1, 40, 2),
    (70, 2, 0.05, 1, 0),
]
ROUTE_MEAN, ROUTE_ONEPASS, ROUTE_GEMM = 0, 1, 2


def _f64_trend(oracle, x, y, h, w, s, xo, degree, c, rho):
    """numpy_trend in float64 on the oracle's Gram, Cholesky and triangular solves."""
    from scipy.linalg import solve_triangular
    Lc = np.asarray(oracle.cho_factor(oracle.gram(x, h, w, s)))
    z = np.asarray(oracle.trsm_lower(Lc, y))
    V = np.asarray(oracle.trsm_lower(Lc, np.asfortranarray(oracle.gram_cross(x, xo, h, w)))).T
    k0 = oracle.kernel_scale(x.shape[0], h, w)
    return numpy_trend(Lc, z, trend_basis(x, degree, c, rho), V, trend_basis(xo, degree, c, rho),
                       k0, solve=lambda Lf, B: np.asarray(oracle.trsm_lower(Lf, B)),
                       solve_t=lambda Lf, B: solve_triangular(Lf, B, lower=True, trans="T"))


def _errors(got, t):
    """The errors of a result {beta, cov_beta, logml_t, alpha_t, mean, var} against the long-double
    dict t, each relative to its scale: a dict of floats."""
    sm, sv, sb, sl = scales(t)
    H, al = t["H"], t["alpha_t"]
    out = {}
    if "beta" in got:
        out["beta"] = float(np.max(np.abs(got["beta"] - t["beta"]).astype(np.float64) / sb))
        out["cov_beta"] = float(np.max(np.abs(got["cov_beta"] - t["cov_beta"]))
                                / np.max(np.abs(t["cov_beta"])))
        out["logml_t"] = float(abs(got["logml_t"] - t["logml_t"])) / sl
        out["alpha_t"] = float(np.max(np.abs(got["alpha_t"] - al)) / np.max(np.abs(al)))
        out["H^T alpha_t"] = float(np.max(np.abs(H.T @ got["alpha_t"].astype(LD))
                                          / (np.abs(H).T @ np.abs(al))))
    if "mean" in got:
        out["mean"] = float(np.max(np.abs(got["mean"] - t["mean"]))) / sm
    if got.get("var") is not None:
        out["var"] = float(np.max(np.abs(got["var"] - t["var"]))) / sv
    return out


def _reference_for(oracle, x, y, h, w, s, xo, degree, label, basis=None):
    """(t, tol): the long-double restatement and, per quantity, 100 max(r, 4 eps) with r the float64
    restatement's error -- both relative to the scales of _errors.  basis: (c, rho), else the
    default one."""
    c, rho = default_basis(x) if basis is None else basis
    t = ld_trend(x, y, h, w, s, xo, degree, c, rho)
    r = _errors(_f64_trend(oracle, x, y, h, w, s, xo, degree, c, rho), t)
    print("%s: r / eps %s" % (label, {k: round(v / EPS, 2) for k, v in r.items()}))
    return t, {k: MARGIN * max(v, 4 * EPS) for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def _reference(oracle, n, d, s, M, degree):
    x, y, h, w, s, xo = _case(n, d, s, M, 1.0)
    return _reference_for(oracle, x, y, h, w, s, xo, degree,
                          "n=%d d=%d M=%d degree=%d" % (n, d, M, degree))


def _as_dict(tr, mv=None):
    out = dict(zip(("beta", "cov_beta", "logml_t", "alpha_t"), tr)) if tr is not None else {}
    if mv is not None:
        out["mean"], out["var"] = mv
    return out


@functools.lru_cache(maxsize=None)
def _device(engine, n, d, s, M, degree):
    """One fit per case: {"trend", "full", "route", "mean_only", "mean_route"}."""
    x, y, h, w, s, xo = _case(n, d, s, M, 1.0)
    c, rho = default_basis(x)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        out = {"full": fit.predict_trend(xo, degree, c, rho), "route": fit.trend_last_route()}
        out["trend"] = fit.trend(degree, c, rho)
        out["mean_only"] = fit.predict_trend(xo, degree, c, rho, want_var=False)
        out["mean_route"] = fit.trend_last_route()
    finally:
        fit.close()
    return out


def _check(got, t, tol, label):
    err = _errors(got, t)
    print("%s: error / tol %s" % (label, {k: round(v / tol[k], 4) for k, v in err.items()}))
    for k, v in err.items():
        assert v <= tol[k], (label, k, v, tol[k])


@pytest.mark.parametrize("n,d,s,M,degree", CASES)
def test_trend_holds_its_contract(engine, oracle, n, d, s, M, degree):
    t, tol = _reference(oracle, n, d, s, M, degree)
    p = trend_p(degree, d)
    label = "n=%d d=%d M=%d degree=%d" % (n, d, M, degree)
    # the conditions that make the comparison mean something, on the reference alone
    sv = scales(t)[1]
    cond = float(np.linalg.cond(t["A"].astype(np.float64)))
    print("%s: cond(A) %.3g, largest r^T A^-1 r / variance scale %.3g"
          % (label, cond, float(np.max(t["quad"])) / sv))
    assert cond <= 1e3
    assert float(np.max(t["quad"])) >= 1e-4 * sv
    dev = _device(engine, n, d, s, M, degree)
    beta, cov, logml, alpha = dev["trend"]
    mean, var = dev["full"]
    assert beta.shape == (p,) and cov.shape == (p, p) and alpha.shape == (n,)
    assert mean.shape == (M,) and var.shape == (M,) and isinstance(logml, float)
    assert np.array_equal(cov, cov.T)
    assert dev["route"][0] == (ROUTE_ONEPASS if p <= 8 else ROUTE_GEMM)
    assert (dev["route"][1] >= 0) == (p > 8)
    _check(_as_dict(dev["trend"], dev["full"]), t, tol, label)


@pytest.mark.parametrize("n,d,s,M,degree", CASES)
def test_mean_only_route_agrees_with_the_full_route(engine, oracle, n, d, s, M, degree):
    t, tol = _reference(oracle, n, d, s, M, degree)
    dev = _device(engine, n, d, s, M, degree)
    mean, var = dev["mean_only"]
    assert var is None and dev["mean_route"] == (ROUTE_MEAN, -1)
    _check({"mean": mean}, t, tol, "mean only n=%d d=%d degree=%d" % (n, d, degree))
    assert float(np.max(np.abs(mean - dev["full"][0]))) <= tol["mean"] * scales(t)[0]


@pytest.mark.parametrize("n,d,s,M,degree", [(200, 3, 0.1, 70, 1), (130, 3, 0.1, 100, 2)])
def test_same_bits_whatever_ran_before_and_the_fit_is_not_disturbed(engine, n, d, s, M, degree):
    x, y, h, w, s, xo = _case(n, d, s, M, 1.0)
    c, rho = default_basis(x)
    fit, fit2 = engine.gp_fit(x, y, h, w, s), engine.gp_fit(x, y, h, w, s)
    try:
        before = fit.predict(xo)[:2] + (fit.alpha(), fit.logml)
        fresh = fit.predict_trend(xo, degree, c, rho)  # the state is computed in this call
        tr = fit.trend(degree, c, rho)                 # ... and is there for this one
        again = fit.predict_trend(xo, degree, c, rho)
        m_only = fit.predict_trend(xo, degree, c, rho, want_var=False)[0]
        after = fit.predict(xo)[:2] + (fit.alpha(), fit.logml)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        assert np.array_equal(fresh[0], again[0]) and np.array_equal(fresh[1], again[1])
        # the other order on a fresh fit: trend first, after a zero-mean prediction
        fit2.predict(xo)
        tr2 = fit2.trend(degree, c, rho)
        late = fit2.predict_trend(xo, degree, c, rho)
        assert np.array_equal(late[0], fresh[0]) and np.array_equal(late[1], fresh[1])
        assert np.array_equal(fit2.predict_trend(xo, degree, c, rho, want_var=False)[0], m_only)
        for a, b in zip(tr, tr2):
            assert np.array_equal(a, b)
        for a, b in zip(tr, fit.trend(degree, c, rho)):
            assert np.array_equal(a, b)
        # the row reductions' own sums are bq_gp_predict's: the one-pass kernel changes none of them
        # (var_t = var + r^T A^-1 r is not below it)
        assert np.all(fresh[1] >= before[1])
    finally:
        fit.close()
        fit2.close()


def test_trend_follows_refit_new_targets_append_and_remove(engine, oracle):
    n, d, s, M, degree = 130, 3, 0.1, 100, 2
    x, y, h, w, s, xo = _case(n, d, s, M, 1.0)
    rs = np.random.RandomState(11)
    fit = engine.gp_fit(x, y, h, w, s)

    def check(x, y, h, w, s, what):
        c, rho = default_basis(x)
        t, tol = _reference_for(oracle, x, y, h, w, s, xo, degree, what)
        got = _as_dict(fit.trend(degree, c, rho), fit.predict_trend(xo, degree, c, rho))
        _check(got, t, tol, what)
        _check({"mean": fit.predict_trend(xo, degree, c, rho, want_var=False)[0]}, t, tol, what)

    try:
        c, rho = default_basis(x)
        fit.trend(degree, c, rho)  # a state that every event below must drop
        h2, w2 = 1.1, w * 1.2
        fit.refit(h2, w2, s)
        check(x, y, h2, w2, s, "after refit")
        y2 = y + 0.3 * rs.randn(n)
        fit.set_y(y2)
        fit.refit(h2, w2, s)
        check(x, y2, h2, w2, s, "after set_y + refit")
        xa, ya = rs.uniform(-3, 3, size=(d, 5)), rs.randn(5)
        fit.append(xa, ya)
        x3, y3 = np.concatenate([x, xa], axis=1), np.concatenate([y2, ya])
        check(x3, y3, h2, w2, s, "after append")
        idx = np.array([3, 64, 131])
        fit.remove(idx)
        check(np.delete(x3, idx, axis=1), np.delete(y3, idx), h2, w2, s, "after remove")
    finally:
        fit.close()


def test_a_second_key_on_the_same_fit(engine, oracle):
    n, d, s, M = 130, 2, 0.05, 130
    x, y, h, w, s, xo = _case(n, d, s, M, 1.0)
    c, rho = default_basis(x)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        first = fit.trend(2, c, rho) + fit.predict_trend(xo, 2, c, rho)
        for degree in (1, 0, 2):
            t, tol = _reference(oracle, n, d, s, M, degree) if degree == 2 else _reference_for(
                oracle, x, y, h, w, s, xo, degree, "degree %d" % degree)
            got = _as_dict(fit.trend(degree, c, rho), fit.predict_trend(xo, degree, c, rho))
            _check(got, t, tol, "second key: degree %d" % degree)
        back = fit.trend(2, c, rho) + fit.predict_trend(xo, 2, c, rho)
        for a, b in zip(first, back):
            assert np.array_equal(a, b)
        # another centre and scale of the same degree: another basis, the same posterior
        c2, rho2 = c + 0.25, rho * 1.5
        t2, tol2 = _reference_for(oracle, x, y, h, w, s, xo, 2, "another basis", (c2, rho2))
        got = _as_dict(fit.trend(2, c2, rho2), fit.predict_trend(xo, 2, c2, rho2))
        assert not np.array_equal(got["beta"], first[0])
        _check(got, t2, tol2, "second key: another centre and scale")
    finally:
        fit.close()


def _raw(engine, fit, degree, c, rho, outs, xo=None):
    """The C entry points on the caller's arrays: the status."""
    from bayesian_quadrature_amd import _lib as L
    c, rho = np.ascontiguousarray(c, dtype=np.float64), np.ascontiguousarray(rho, dtype=np.float64)
    if xo is None:
        return engine._lib.bq_gp_trend(engine._ctx, fit._handle(), degree, L.dptr(c), L.dptr(rho),
                                       *[L.dptr(o) for o in outs])
    M = xo if isinstance(xo, int) else xo.shape[1]
    return engine._lib.bq_gp_predict_trend(engine._ctx, fit._handle(), degree, L.dptr(c),
                                           L.dptr(rho), None if isinstance(xo, int) else L.dptr(xo),
                                           M, *[L.dptr(o) for o in outs])


def test_coincident_points_are_not_positive_definite_and_nothing_is_written(engine):
    from bayesian_quadrature_amd import _lib as L
    x = np.asfortranarray(np.zeros((2, 6)) + np.array([[0.3], [-0.2]]))
    y = np.arange(6.0)
    c, rho = np.array([0.3, -0.2]), np.array([1.0, 1.0])
    xo = np.asfortranarray(np.random.RandomState(0).uniform(-1, 1, size=(2, 70)))
    fit = engine.gp_fit(x, y, 1.3, np.array([0.8, 0.9]), 0.1)
    try:
        outs = [np.full(6, -7.5), np.full(36, -7.5), np.full(1, -7.5), np.full(6, -7.5)]
        assert _raw(engine, fit, 2, c, rho, outs) == L.BQ_ERR_NOT_PD
        assert all(np.all(o == -7.5) for o in outs)
        for mv in ([np.full(70, -7.5), np.full(70, -7.5)], [np.full(70, -7.5), None]):
            assert _raw(engine, fit, 2, c, rho, mv, xo) == L.BQ_ERR_NOT_PD
            assert all(o is None or np.all(o == -7.5) for o in mv)
        with pytest.raises(np.linalg.LinAlgError):
            fit.trend(2, c, rho)
        with pytest.raises(np.linalg.LinAlgError):
            fit.predict_trend(xo, 2, c, rho)
        # the fit is what it was, and a basis it supports is served
        beta, cov, logml, alpha = fit.trend(0, c, rho)
        assert np.isfinite(beta[0]) and cov[0, 0] > 0 and np.isfinite(logml)
        m, v = fit.predict_trend(xo, 0, c, rho)
        assert np.all(np.isfinite(m)) and np.all(v >= fit.predict(xo)[1])
    finally:
        fit.close()


def test_argument_rules_on_the_device(engine):
    from bayesian_quadrature_amd import _lib as L
    x, y, h, w, s, xo = _case(65, 3, 0.1, 8, 1.0)
    c, rho = default_basis(x)
    fit, small = engine.gp_fit(x, y, h, w, s), engine.gp_fit(x[:, :9], y[:9], h, w, s)
    try:
        def outs():
            return [np.full(10, -7.5), np.full(100, -7.5), np.full(1, -7.5), np.full(65, -7.5)]

        def bad(st, o):
            assert st == L.BQ_ERR_BAD_ARG and all(a is None or np.all(a == -7.5) for a in o)

        for degree in (-1, 3):
            o = outs()
            bad(_raw(engine, fit, degree, c, rho, o), o)
        for v in (np.nan, np.inf):
            cc = c.copy()
            cc[1] = v
            o = outs()
            bad(_raw(engine, fit, 2, cc, rho, o), o)
        for v in (0.0, -1.0, np.nan, np.inf):
            rr = rho.copy()
            rr[2] = v
            o = outs()
            bad(_raw(engine, fit, 2, c, rr, o), o)
            mv = [np.full(8, -7.5), np.full(8, -7.5)]
            bad(_raw(engine, fit, 2, c, rr, mv, xo), mv)
        o = outs()
        bad(_raw(engine, small, 2, c, rho, o), o)  # n = 9 < p = 10
        assert _raw(engine, small, 1, c, rho, outs()) == L.BQ_OK
        bad(_raw(engine, fit, 2, c, rho, [None, None, None, None]), [])
        bad(_raw(engine, fit, 2, c, rho, [None, None], xo), [])
        mv = [np.full(8, -7.5), np.full(8, -7.5)]
        bad(_raw(engine, fit, 2, c, rho, mv, -1), mv)
        assert _raw(engine, fit, 2, c, rho, mv, 0) == L.BQ_OK and np.all(mv[0] == -7.5)
        assert fit.trend_last_route() == (-1, -1)  # nothing above reached the device
        fit.set_y(y + 1.0)
        o = outs()
        bad(_raw(engine, fit, 2, c, rho, o), o)  # new targets: refit required
    finally:
        fit.close()
        small.close()
