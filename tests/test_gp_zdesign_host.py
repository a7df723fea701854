"""CPU tests of the integral of a fit and of the designs that lower its variance: the contracts of
bq_gp_integral and bq_gp_zdesign restated in numpy (``numpy_integral``, ``numpy_zdesign``), their
properties checked on the restatements alone, and the host plumbing -- engine.Fit.integral and
engine.Fit.integral_design as gp.GP.integral*, BQ.l_integral and BQ.l_integral_design use them --
over the oracle-backed engine double with both built on ``predict(want_cov=True)`` and the
oracle's ``int_K``.  test_gp_zdesign.py holds the device to the same contracts."""
import pickle

import numpy as np
import pytest

from engine_double import EngineDouble
from test_gp_ivr_host import numpy_ivr
from test_gp_pivchol_host import OPTIONS, PivcholFitDouble, _data
from test_gp_sample_host import kernel_scale


def numpy_integral(kap_x, Kxx, y, kk):
    """(mean, var, weights): the contract of bq_gp_integral from the kernel means at the fit's
    points, Kxx = K + s^2 I, the targets and kk = int int k, in the arrays' own precision:
    b = L^-1 kappa_X, mean = b . z, var = kk - b . b (not clamped), weights = L^-T b."""
    kap_x, Kxx, y = np.asarray(kap_x), np.asarray(Kxx), np.asarray(y)
    L = np.linalg.cholesky(Kxx)
    b, z = np.linalg.solve(L, kap_x), np.linalg.solve(L, y)
    return b @ z, kk - b @ b, np.linalg.solve(L.T, b)


def numpy_zdesign(Sigma_cc, u0, zvar0, kk, k0, q, nugget=0.0, tol=0.0, pivots=None):
    """(piv (q, -1 from rank on), gain (q), zvar0, resid_u, resid_c, score0, rank): the contract
    of bq_gp_zdesign on a given covariance over the A candidates and u0 = Cov(Z, f(xc) | data), in
    the covariance's own precision.  kk, the prior variance of Z, scales the stop level; k0 is
    taken only so that calls read like ``numpy_ivr``'s.  pivots: take these instead of the argmax
    (the recurrence along another call's choices); the stop rule still applies."""
    Sigma = np.asarray(Sigma_cc)
    dt = Sigma.dtype
    A = Sigma.shape[0]
    u = np.array(u0, dtype=dt)
    if q < 1 or (A and q > A) or u.shape != (A,) or \
            not (np.isfinite(nugget) and nugget >= 0) or not (np.isfinite(tol) and tol >= 0):
        raise ValueError("illegal value")
    nu = dt.type(nugget)
    dc = np.array(np.diag(Sigma), dtype=dt)
    C = np.zeros((A, q), dtype=dt)
    piv, gain = np.full(q, -1, dtype=np.int64), np.zeros(q, dtype=dt)
    taken = np.zeros(A, dtype=bool)
    score0 = np.zeros(A, dtype=dt)
    rank = q
    for t in range(q):
        den2 = dc + nu
        ok = (den2 > 0) & ~taken if nugget == 0 else den2 > 0
        score = np.zeros(A, dtype=dt)
        with np.errstate(invalid="ignore", over="ignore"):  # (such a score stops the run below)
            score[ok] = u[ok] * u[ok] / den2[ok]
        if t == 0:
            score0 = score.copy()
        cand = np.flatnonzero(ok)
        if pivots is not None:
            p = int(pivots[t])
            g = score[p] if ok[p] else dt.type(-np.inf)
        elif cand.size == 0:
            p, g = -1, dt.type(-np.inf)
        elif np.any(np.isnan(score[cand])):  # a NaN comes first and stops the run
            p, g = int(cand[np.flatnonzero(np.isnan(score[cand]))[0]]), dt.type(np.nan)
        else:
            p = int(cand[np.argmax(score[cand])])  # the first of equals
            g = score[p]
        if not (g > tol * kk and g > 0 and np.isfinite(g)):
            rank = t
            break
        den = np.sqrt(dc[p] + nu)
        c = (Sigma[:, p] - C[:, :t] @ C[p, :t]) / den
        coef = u[p] / den
        if nugget == 0:
            c[taken] = 0
            c[p] = den
            taken[p] = True
        u = u - c * coef
        dc = dc - c * c
        if nugget == 0:
            dc[taken] = 0
            u[taken] = 0
        C[:, t] = c
        piv[t], gain[t] = p, g
    return piv, gain, zvar0, u, dc, score0, rank


def zvar_after(Sigma_cc, u0, zvar0, P, nugget):
    """var Z with the candidates P observed with noise ``nugget``, from the definition."""
    P = np.asarray(P, dtype=np.int64)
    if P.size == 0:
        return zvar0
    S = Sigma_cc[np.ix_(P, P)] + nugget * np.eye(P.size)
    return zvar0 - u0[P] @ np.linalg.solve(S, u0[P])


class ZdFitDouble(PivcholFitDouble):
    """The engine double's fit with ``integral`` and ``integral_design`` (and ``ivr_design``, for
    the demonstration) over the oracle."""

    def _pts(self, a):
        a = np.asarray(a, dtype=np.float64)
        a = a[None, :] if a.ndim == 1 else a
        if a.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        return a

    def _measure(self, mu, cov):
        mu = np.atleast_1d(np.asarray(mu, dtype=np.float64))
        cov = np.atleast_2d(np.asarray(cov, dtype=np.float64))
        if not (np.all(np.isfinite(mu)) and np.all(np.isfinite(cov))):
            raise ValueError("the measure must be finite")
        try:
            np.linalg.cholesky(cov + np.diag(self.w ** 2))
        except np.linalg.LinAlgError:
            raise ValueError("the measure's covariance plus diag(w^2) is not positive definite")
        return mu, cov

    def integral(self, mu, cov, want_weights=False):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        mu, cov = self._measure(mu, cov)
        self.calls.append(("integral", mu.copy(), cov.copy(), want_weights, self.h))
        kap = self.o.int_K(self.x, self.h, self.w, mu, cov)
        kk = float(self.o.int_int_K(self.d, self.h, self.w, mu, cov))
        mean, var, wts = numpy_integral(kap, self.K(), self.y, kk)
        res = (float(mean), float(var))
        return res + (wts,) if want_weights else res

    def _u0(self, xc, mu, cov):
        kap = self.o.int_K(self.x, self.h, self.w, mu, cov)
        wts = np.linalg.solve(np.asarray(self.K()), kap)
        Kcx = np.asarray(self.o.gram_cross(xc if self.d > 1 else xc[0], self.x, self.h, self.w))
        kc = self.o.int_K(xc if self.d > 1 else xc[0], self.h, self.w, mu, cov)
        kk = float(self.o.int_int_K(self.d, self.h, self.w, mu, cov))
        return kc - Kcx @ wts, kk - kap @ wts, kk

    def integral_design(self, xc, q, mu, cov, nugget=0.0, tol=0.0, want_scores=False):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        xc = self._pts(xc)
        mu, cov = self._measure(mu, cov)
        self.calls.append(("zdesign", xc.shape[1], q, nugget, tol, self.h, mu.copy(), cov.copy()))
        u0, zvar0, kk = self._u0(xc, mu, cov)
        _, _, Sig = self.predict(xc if self.d > 1 else xc[0], want_cov=True)
        piv, gain, zvar0, ru, rc, s0, r = numpy_zdesign(
            np.asarray(Sig), u0, float(zvar0), kk, kernel_scale(self.h, self.w), q, nugget, tol)
        res = (piv[:r], gain[:r], float(zvar0), ru, rc)
        return res + (s0,) if want_scores else res

    def ivr_design(self, xc, q, xr=None, rho=None, nugget=0.0, tol=0.0, want_scores=False):
        assert xr is None
        xc = self._pts(xc)
        _, _, cov = self.predict(xc[0], want_cov=True)
        piv, gain, ivar0, rr, rc, s0, r = numpy_ivr(np.asarray(cov), 0, rho,
                                                    kernel_scale(self.h, self.w), q, nugget, tol)
        return piv[:r], gain[:r], float(ivar0), rr, rc


class ZdEngineDouble(EngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return ZdFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def pkg(oracle):
    import bayesian_quadrature_amd as pkg
    from bayesian_quadrature_amd import engine as eng_mod
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(ZdEngineDouble(oracle), 0)
    yield pkg
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _case(A=18, n=10, s=0.3, seed=0, width=0.8, mu=0.4, sig=1.3):
    """A 1-D posterior in float64 over A candidates under the measure N(mu, sig^2): (Sigma_cc, u0,
    zvar0, kk, k0), everything from the definitions."""
    rs = np.random.RandomState(seed)
    x, xc = rs.uniform(-3, 3, n), rs.uniform(-3, 3, A)

    def k(a, b):
        return np.exp(-0.5 * (a[:, None] - b[None, :]) ** 2 / width ** 2)

    def kap(a):  # int k(a, x') N(x' | mu, sig^2) dx' for this unnormalised kernel
        v = width ** 2 + sig ** 2
        return width / np.sqrt(v) * np.exp(-0.5 * (a - mu) ** 2 / v)

    kk = width / np.sqrt(width ** 2 + 2 * sig ** 2)
    Kxx = k(x, x) + s * s * np.eye(n)
    Kcx = k(xc, x)
    Sig = k(xc, xc) - Kcx @ np.linalg.solve(Kxx, Kcx.T)
    wts = np.linalg.solve(Kxx, kap(x))
    return Sig, kap(xc) - Kcx @ wts, kk - kap(x) @ wts, kk, 1.0


# ---- the restatements alone ----

@pytest.mark.parametrize("nu", [0.0, 0.09])
def test_restatement_gains_telescope_and_prefixes(nu):
    """var Z drops by exactly the gain at every step: a j-step run leaves zvar0 less its j gains,
    which is var Z recomputed from scratch with the chosen points observed, and the runs are
    prefixes of one another."""
    Sig, u0, zvar0, kk, k0 = _case()
    full = numpy_zdesign(Sig, u0, zvar0, kk, k0, 8, nu)
    assert full[6] == 8 and np.all(full[1] > 0)
    for j in range(1, 9):
        piv, gain, z0, ru, rc, s0, rank = numpy_zdesign(Sig, u0, zvar0, kk, k0, j, nu)
        assert rank == j and np.array_equal(piv, full[0][:j]) and np.array_equal(gain, full[1][:j])
        assert z0 == zvar0 and np.array_equal(s0, full[5])
        assert abs(zvar_after(Sig, u0, zvar0, piv, nu) - (zvar0 - gain.sum())) <= 1e-13 * kk
        # the residuals are the posterior's after the observations
        P = piv
        G = np.linalg.solve(Sig[np.ix_(P, P)] + nu * np.eye(j), Sig[P, :])
        assert np.allclose(rc, np.diag(Sig - Sig[:, P] @ G), rtol=0, atol=1e-12)
        assert np.allclose(ru, u0 - G.T @ u0[P], rtol=0, atol=1e-12)
    assert full[5][full[0][0]] == full[1][0] == full[5].max()
    assert zvar0 - full[1].sum() > 0


@pytest.mark.parametrize("nu", [0.0, 0.09])
def test_restatement_first_pivot_is_the_best_single_observation(nu):
    Sig, u0, zvar0, kk, k0 = _case(seed=2)
    left = [zvar_after(Sig, u0, zvar0, [a], nu) for a in range(Sig.shape[0])]
    piv, gain, z0, ru, rc, s0, rank = numpy_zdesign(Sig, u0, zvar0, kk, k0, 1, nu)
    assert piv[0] == int(np.argmin(left))
    assert np.allclose(zvar0 - s0, left, rtol=0, atol=1e-14)


def test_restatement_taken_rows_without_a_nugget():
    Sig, u0, zvar0, kk, k0 = _case()
    piv, gain, z0, ru, rc, s0, rank = numpy_zdesign(Sig, u0, zvar0, kk, k0, 12, 0.0)
    assert rank == 12 and len(set(piv.tolist())) == 12
    assert np.all(ru[piv] == 0.0) and np.all(rc[piv] == 0.0)
    # with a large nugget the best candidate is taken again and nothing is zeroed
    piv, gain, z0, ru, rc, s0, rank = numpy_zdesign(Sig, u0, zvar0, kk, k0, 12, 2.0)
    assert rank == 12 and len(set(piv.tolist())) < 12 and np.all(rc > 0)


def test_restatement_tie_rule_stop_rule_and_nan_rule():
    Sig = np.diag([1.0, 2.0, 2.0, 0.5])
    u0 = np.array([1.0, 2.0, 2.0, 0.25])
    piv, gain, z0, ru, rc, s0, rank = numpy_zdesign(Sig, u0, 10.0, 10.0, 1.0, 4)
    assert list(piv) == [1, 2, 0, 3] and rank == 4  # the lowest index among equals
    assert np.array_equal(gain, [2.0, 2.0, 1.0, 0.125])
    assert np.all(rc == 0.0) and np.all(ru == 0.0)
    # with a nugget the best candidate may be taken again
    assert list(numpy_zdesign(np.diag([4.0, 0.1]), np.array([4.0, 0.01]), 9.0, 9.0, 1.0, 2,
                              nugget=1.0)[0]) == [0, 0]
    # nothing to gain: u = 0
    out = numpy_zdesign(Sig, np.zeros(4), 1.0, 1.0, 1.0, 3)
    assert out[6] == 0 and np.all(out[0] == -1) and np.all(out[1] == 0.0)
    assert np.array_equal(out[4], np.diag(Sig)) and np.all(out[5] == 0.0)
    # no eligible candidate; a score that is not finite
    assert numpy_zdesign(np.zeros((3, 3)), np.ones(3), 1.0, 1.0, 1.0, 2)[6] == 0
    assert numpy_zdesign(np.eye(2), np.array([1.0, np.inf]), 1.0, 1.0, 1.0, 2)[6] == 0
    # a NaN comes first and stops the run, whatever the other scores are
    out = numpy_zdesign(np.eye(3), np.array([5.0, np.nan, 7.0]), 1.0, 1.0, 1.0, 2)
    assert out[6] == 0 and np.all(out[0] == -1) and np.isnan(out[5][1])
    # a stop level between the smallest gain and every gain before it ends the run there (the
    # gains of this design need not fall from step to step)
    Sg, u0, zvar0, kk, k0 = _case()
    full = numpy_zdesign(Sg, u0, zvar0, kk, k0, 8)
    j = int(np.argmin(full[1]))
    assert j >= 2
    level = np.sqrt(full[1][j] * full[1][:j].min()) / kk
    out = numpy_zdesign(Sg, u0, zvar0, kk, k0, 8, tol=level)
    assert out[6] == j and np.array_equal(out[0][:j], full[0][:j]) and np.all(out[0][j:] == -1)
    assert np.array_equal(out[1][:j], full[1][:j]) and np.all(out[1][j:] == 0.0)
    # along given pivots the recurrence follows them
    alt = numpy_zdesign(Sg, u0, zvar0, kk, k0, 3, pivots=[5, 1, 7])
    assert list(alt[0]) == [5, 1, 7] and alt[1][0] == full[5][5]


def test_restatement_argument_errors():
    Sig, u0, zvar0, kk, k0 = _case(A=4)
    for bad in (dict(q=0), dict(q=5), dict(q=2, nugget=-1.0), dict(q=2, nugget=np.nan),
                dict(q=2, tol=-1e-3), dict(q=2, tol=np.inf)):
        with pytest.raises(ValueError):
            numpy_zdesign(Sig, u0, zvar0, kk, k0, **bad)
    with pytest.raises(ValueError):
        numpy_zdesign(Sig, u0[:3], zvar0, kk, k0, 2)


def test_integral_agrees_with_the_trapezoid_rule(oracle):
    """mean = int mean(x) pi(x) dx and var = int int cov(x, x') pi(x) pi(x') dx dx' on a 1-D grid,
    to the accuracy test_oracle_known_answers.py holds its trapezoid checks to (atol 1e-7)."""
    import scipy.stats
    x, y = _data(n=12)
    h, w, s, mu, sig = 1.2, 0.8, 0.2, 0.3, 1.1
    fit = ZdFitDouble(oracle, x, y, h, w, s)
    mean, var, wts = fit.integral([mu], [[sig ** 2]], want_weights=True)
    xo = np.linspace(-12.0, 12.0, 1601)
    p = scipy.stats.norm.pdf(xo, mu, sig)
    m, _, cov = fit.predict(xo, want_cov=True)
    assert abs(mean - np.trapezoid(m * p, xo)) <= 1e-7
    assert abs(var - np.trapezoid(np.trapezoid(np.asarray(cov) * p[None, :], xo, axis=1) * p,
                                  xo)) <= 1e-7
    assert var > 0 and abs(wts @ y - mean) <= 1e-12 * np.abs(wts).dot(np.abs(y))


# ---- the demonstration ----

def test_integral_design_leaves_the_least_variance_of_the_integral(pkg):
    """test_gp_ivr_host.py's setting: 33 candidates on [-4, 4], the measure N(0, 1), six noisy
    picks each.  The max-variance design leaves 99.9 % of var Z, the design that minimises the
    integrated variance (the candidates as reference points, N(0, 1) weights) 82.3 %, this design
    75.5 %: this <= ivr <= max-variance holds here, and is all that is asserted."""
    import scipy.stats
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.linspace(-4.0, 4.0, 33)
    rho = scipy.stats.norm.pdf(xo)
    rho /= rho.sum()
    mu, cov, nu = [0.0], [[1.0]], 0.2 ** 2
    idx, info = g.integral_design(xo, 6, mu, cov, return_info=True)
    mid = g.ivr_design(xo, 6, weights=rho)
    far = g.greedy_design(xo, 6)
    Sig = np.asarray(g._fit.predict(xo, want_cov=True)[2])
    u0, zvar0, kk = g._fit._u0(xo[None, :], np.array(mu), np.array(cov))
    left = [zvar_after(Sig, u0, zvar0, P, nu) / zvar0 for P in (idx, mid, far)]
    print("var Z left: this %.4f (at %s), ivr %.4f (at %s), max-variance %.4f (at %s)"
          % (left[0], xo[idx], left[1], xo[mid], left[2], xo[far]))
    assert abs(zvar0 - info["zvar0"]) <= 1e-14 and abs(zvar0 - g.integral(mu, cov)[1]) <= 1e-14
    assert abs(left[0] - (zvar0 - info["gain"].sum()) / zvar0) <= 1e-12
    assert left[0] <= left[1] <= left[2]


# ---- the plumbing ----

def test_signatures_are_declared():
    from bayesian_quadrature_amd import _lib
    import ctypes as C
    res, args = _lib.SIGNATURES["bq_gp_integral"]
    assert res is C.c_int and len(args) == 7
    assert args[0] is C.c_void_p and args[1] is C.c_void_p and all(a is _lib._dp for a in args[2:])
    res, args = _lib.SIGNATURES["bq_gp_zdesign"]
    assert res is C.c_int and len(args) == 16
    assert args[0] is C.c_void_p and args[1] is C.c_void_p
    assert all(args[i] is _lib._dp for i in (2, 3, 4, 10, 11, 12, 13, 14))
    assert args[5] is C.c_int64 and args[6] is C.c_int64
    assert args[7] is C.c_double and args[8] is C.c_double
    assert args[9] is _lib._i64p and args[15] is _lib._i64p


def test_gp_integral_shapes_memoisation_and_invalidation(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    mean, var = g.integral(0.3, 1.21)
    assert isinstance(mean, float) and isinstance(var, float) and var > 0
    fit = g._fit
    n_calls = len(fit.calls)
    assert g.integral([0.3], [[1.21]]) == (mean, var)  # the same measure in another spelling
    wts = g.integral_weights(0.3, 1.21)
    assert wts.shape == (40,) and abs(wts @ y - mean) <= 1e-12 * np.abs(wts).dot(np.abs(y))
    wts[0] = 7.0  # a copy: the memoised weights stay
    assert g.integral_weights(0.3, 1.21)[0] != 7.0
    assert len(fit.calls) == n_calls  # memoised: one device call for all of it
    assert fit.calls[-1][0] == "integral" and fit.calls[-1][3] is True
    # another measure is another entry
    other = g.integral(0.0, 1.0)
    assert other != (mean, var) and len(fit.calls) == n_calls + 1
    assert g.integral(0.3, 1.21) == (mean, var) and len(fit.calls) == n_calls + 1
    # a parameter change refits and recomputes
    g.set_param("h", 1.3)
    m2, v2 = g.integral(0.3, 1.21)
    assert g._fit is fit and fit.calls[-1][4] == 1.3 and len(fit.calls) == n_calls + 2
    assert (m2, v2) != (mean, var)
    # new targets: the variance and the weights do not depend on them
    w2 = g.integral_weights(0.3, 1.21)
    g.y = 2.0 * y
    m3, v3 = g.integral(0.3, 1.21)
    assert abs(m3 - 2.0 * m2) <= 1e-12 * abs(m2) and abs(v3 - v2) <= 1e-14
    assert np.allclose(g.integral_weights(0.3, 1.21), w2, rtol=1e-12, atol=0)
    # new data
    g.x = x + 0.01
    assert g.integral(0.3, 1.21) != (m3, v3)


def test_gp_integral_design_shapes_and_noisy(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.linspace(-2.9, 2.9, 17)
    mu, cov = np.array([0.3]), np.array([[1.21]])
    idx = g.integral_design(xo, 5, 0.3, 1.21)
    assert idx.shape == (5,) and idx.dtype == np.int64
    call = g._fit.calls[-1]
    assert call[:5] == ("zdesign", 17, 5, 0.2 ** 2, 0.0)  # noisy by default: nugget = s^2
    assert np.array_equal(call[6], mu) and np.array_equal(call[7], cov)
    Sig = np.asarray(g._fit.predict(xo, want_cov=True)[2])
    u0, zvar0, kk = g._fit._u0(xo[None, :], mu, cov)
    k0 = kernel_scale(1.2, 0.8)
    want = numpy_zdesign(Sig, u0, zvar0, kk, k0, 5, nugget=0.2 ** 2)
    assert np.array_equal(idx, want[0])
    idx2, info = g.integral_design(xo[None, :], 5, mu, cov, return_info=True)
    assert set(info) == {"gain", "zvar0", "resid", "resid_u"} and np.array_equal(idx2, idx)
    assert info["gain"].shape == (5,) and np.array_equal(info["gain"], want[1])
    assert info["zvar0"] == want[2] and isinstance(info["zvar0"], float)
    assert abs(info["zvar0"] - g.integral(mu, cov)[1]) <= 1e-14
    assert info["resid"].shape == (17,) and info["resid_u"].shape == (17,)
    assert np.array_equal(info["resid"], want[4]) and np.array_equal(info["resid_u"], want[3])
    # not noisy: no nugget, no candidate twice, exact zeros; a stop level is passed on
    idx3, info3 = g.integral_design(xo, 5, mu, cov, noisy=False, tol=1e-9, return_info=True)
    assert g._fit.calls[-1][3:5] == (0.0, 1e-9) and len(set(idx3.tolist())) == 5
    assert np.all(info3["resid"][idx3] == 0.0) and np.all(info3["resid_u"][idx3] == 0.0)
    # a stop level above every gain: nothing chosen
    idx4, info4 = g.integral_design(xo, 5, mu, cov, tol=10.0, return_info=True)
    assert idx4.shape == (0,) and info4["gain"].shape == (0,) and info4["zvar0"] == want[2]
    # the surface is step 0's scores
    sc = g.integral_scores(xo, mu, cov)
    assert sc.shape == (17,) and np.array_equal(sc, want[5]) and g._fit.calls[-1][2] == 1
    assert int(np.argmax(sc)) == idx[0]
    assert np.array_equal(g.integral_scores(xo, mu, cov, noisy=False),
                          numpy_zdesign(Sig, u0, zvar0, kk, k0, 1)[5])
    # empty candidates: nothing chosen, the variance before is still there
    for e in ([], np.empty(0), np.empty((1, 0))):
        idx5, info5 = g.integral_design(e, 3, mu, cov, return_info=True)
        assert idx5.shape == (0,) and idx5.dtype == np.int64
        assert abs(info5["zvar0"] - want[2]) <= 1e-14
        assert all(info5[k].shape == (0,) for k in ("gain", "resid", "resid_u"))
        assert g.integral_scores(e, mu, cov).shape == (0,)


def test_gp_integral_argument_errors(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.array([0.1, 0.5, -2.0])
    for q in (0, -1, 4):
        with pytest.raises(ValueError):
            g.integral_design(xo, q, 0.0, 1.0)
    for tol in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError):
            g.integral_design(xo, 2, 0.0, 1.0, tol=tol)
    for mu, cov in (([0.0, 1.0], 1.0), (0.0, np.eye(2)), (np.nan, 1.0), (0.0, np.inf),
                    (0.0, -5.0)):
        with pytest.raises(ValueError):
            g.integral(mu, cov)
        with pytest.raises(ValueError):
            g.integral_weights(mu, cov)
        with pytest.raises(ValueError):
            g.integral_design(xo, 2, mu, cov)
        with pytest.raises(ValueError):
            g.integral_scores(xo, mu, cov)
    with pytest.raises(ValueError):
        g.integral_design(np.zeros((2, 3)), 2, 0.0, 1.0)  # dimension mismatch with the fit
    assert g.integral_design(xo, 3, 0.0, 1.0).shape == (3,)


def test_gp_integral_survives_pickling(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    a = g.integral(0.3, 1.21)
    g2 = pickle.loads(pickle.dumps(g))
    assert g2._memoized == {} and g2._fit is None  # only data and parameters travel
    assert g2.integral(0.3, 1.21) == a
    xo = np.linspace(-2, 2, 9)
    assert np.array_equal(g2.integral_design(xo, 3, 0.3, 1.21), g.integral_design(xo, 3, 0.3, 1.21))


def _bq(pkg, kernel=None):
    import scipy.stats
    np.random.seed(8728)
    x = np.linspace(-5, 5, 9)
    bq = pkg.BQ(x, scipy.stats.norm.pdf(x, 0, 1), kernel=kernel or pkg.GaussianKernel, **OPTIONS)
    return bq


def test_bq_l_integral_and_design(pkg):
    bq = _bq(pkg)
    bq.init(params_tl=(15, 2, 0.1), params_l=(0.2, 1.3, 0))
    mean, var = bq.l_integral()
    assert np.allclose(mean, bq.Z_mean())
    assert var >= 0 or abs(var) < 1e-12
    assert (mean, var) == bq.gp_l.integral(bq.options["x_mean"], bq.options["x_cov"])
    x_c = np.linspace(-7, 7, 29)
    idx = bq.l_integral_design(x_c, 4)
    assert idx.shape == (4,) and idx.dtype == np.int64
    call = bq.gp_l._fit.calls[-1]
    assert call[:4] == ("zdesign", 29, 4, 0.0)  # gp_l carries no noise
    assert np.array_equal(call[6], [OPTIONS["x_mean"]]) and np.array_equal(call[7], [[OPTIONS["x_var"]]])
    assert np.array_equal(idx, bq.gp_l.integral_design(x_c, 4, OPTIONS["x_mean"], OPTIONS["x_var"]))
    assert bq.l_integral_design([], 4).shape == (0,)


def test_bq_l_integral_raises_on_the_approximate_branch(pkg):
    bq = _bq(pkg, pkg.PeriodicKernel)
    assert bq.options["use_approx"]
    with pytest.raises(NotImplementedError):
        bq.l_integral()
    with pytest.raises(NotImplementedError):
        bq.l_integral_design(np.array([0.1, 0.2]), 1)
