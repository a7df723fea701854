"""CPU tests of the pivoted partial Cholesky of a posterior: the contract of bq_gp_pivchol restated
in numpy on a given covariance (``numpy_pivchol``), its properties checked on the restatement
alone, and the host plumbing -- engine.Fit.pivoted_cholesky's contract as gp.GP.pivoted_cholesky,
gp.GP.greedy_design and BQ.log_l_design use it -- over the oracle-backed engine double with a
``pivoted_cholesky`` built on ``predict(want_cov=True)``.  test_gp_pivchol.py holds the device to
the same contract."""
import numpy as np
import pytest

from engine_double import EngineDouble, FitDouble
from test_gp_sample_host import kernel_scale


def numpy_pivchol(Sigma, k0, q, nugget=0.0, tol=0.0, pivots=None):
    """(piv (q, -1 from rank on), C (M, q), resid (M,), gain (q), rank): the contract of
    bq_gp_pivchol on a given covariance, in the covariance's own precision.  pivots: take these
    instead of the argmax (the recurrence along another call's choices); the stop rule still
    applies."""
    Sigma = np.asarray(Sigma)
    M = Sigma.shape[0]
    if q < 1 or q > M or not (np.isfinite(nugget) and nugget >= 0) or \
            not (np.isfinite(tol) and tol >= 0):
        raise ValueError("illegal value")
    dt = Sigma.dtype
    d = np.array(np.diag(Sigma), dtype=dt)
    C = np.zeros((M, q), dtype=dt, order="F")
    piv, gain = np.full(q, -1, dtype=np.int64), np.zeros(q, dtype=dt)
    taken = np.zeros(M, dtype=bool)
    rank = q
    for j in range(q):
        p = int(np.argmax(d)) if pivots is None else int(pivots[j])  # the first of equals
        g = d[p]
        if not (g > tol * k0 and g > 0 and np.isfinite(g)):
            rank = j
            break
        den = np.sqrt(g + dt.type(nugget))
        c = (Sigma[:, p] - C[:, :j] @ C[p, :j]) / den
        if nugget == 0:
            c[taken] = 0
            c[p] = den
            taken[p] = True
        d = d - c * c
        if nugget == 0:
            d[taken] = 0
        C[:, j] = c
        piv[j], gain[j] = p, g
    return piv, C, d, gain, rank


class PivcholFitDouble(FitDouble):
    def __init__(self, *args):
        self.calls = []
        FitDouble.__init__(self, *args)

    def pivoted_cholesky(self, xo, q, nugget=0.0, tol=0.0, want_factor=True):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        xo = np.asarray(xo, dtype=np.float64)
        xo = xo[None, :] if xo.ndim == 1 else xo
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        self.calls.append(("pivchol", xo.shape[1], q, nugget, tol, self.h))
        _, _, cov = self.predict(xo, want_cov=True)
        piv, C, resid, gain, r = numpy_pivchol(np.asarray(cov), kernel_scale(self.h, self.w), q,
                                               nugget, tol)
        return piv[:r], (np.asfortranarray(C[:, :r]) if want_factor else None), resid, gain[:r]


class PivcholEngineDouble(EngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return PivcholFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def pkg(oracle):
    import bayesian_quadrature_amd as pkg
    from bayesian_quadrature_amd import engine as eng_mod
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(PivcholEngineDouble(oracle), 0)
    yield pkg
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _sigma(M=30, n=12, s=0.3, seed=0, width=0.8):
    """A posterior covariance in float64: k(xo, xo) - k(xo, x) (k(x, x) + s^2 I)^-1 k(x, xo)."""
    rs = np.random.RandomState(seed)
    x, xo = rs.uniform(-3, 3, n), rs.uniform(-3, 3, M)

    def k(a, b):
        return np.exp(-0.5 * (a[:, None] - b[None, :]) ** 2 / width ** 2)

    Kox = k(xo, x)
    return k(xo, xo) - Kox @ np.linalg.solve(k(x, x) + s * s * np.eye(n), Kox.T), 1.0


def _data(n=40, seed=3):
    rs = np.random.RandomState(seed)
    x = np.sort(rs.uniform(-3, 3, size=n))
    return x, np.sin(x) + 0.1 * rs.randn(n)


# ---- the restatement alone ----

def test_restatement_exact_factor_without_nugget():
    Sig, k0 = _sigma()
    M = Sig.shape[0]
    piv, C, resid, gain, rank = numpy_pivchol(Sig, k0, 10)
    assert rank == 10 and len(set(piv)) == 10
    P = piv[:rank]
    assert np.allclose(C @ C[P].T, Sig[:, P], rtol=0, atol=1e-13)
    assert np.all(C[P][np.triu_indices(rank, 1)] == 0.0)
    assert np.array_equal(np.diag(C[P]), np.sqrt(gain))
    assert np.all(resid[P] == 0.0)
    assert np.allclose(resid, np.diag(Sig) - np.sum(C * C, axis=1), rtol=0, atol=1e-14)
    assert np.all(np.diff(gain) <= 1e-14)  # greedy gains of a PSD matrix do not grow
    # a full factorisation gives the matrix back
    piv, C, resid, gain, rank = numpy_pivchol(Sig + 1e-6 * np.eye(M), k0, M)
    assert rank == M and sorted(piv) == list(range(M))
    assert np.allclose(C @ C.T, Sig + 1e-6 * np.eye(M), rtol=0, atol=1e-13)


@pytest.mark.parametrize("nu", [0.09, 1e-3, 2.0])
def test_restatement_resid_is_the_variance_after_noisy_observations(nu):
    """With a nugget the running variances are the posterior variances after noisy observations at
    the pivots: resid = diag(Sigma - Sigma[:, P] (Sigma[P, P] + nu I)^-1 Sigma[P, :]), P with its
    repeats.  And with L the lower triangle of C[P, :] whose diagonal is sqrt(gain + nu):
    L L^T = Sigma[P, P] + nu I and C L^T = Sigma[:, P]."""
    Sig, k0 = _sigma(M=25)
    q = 20
    piv, C, resid, gain, rank = numpy_pivchol(Sig, k0, q, nugget=nu)
    assert rank == q
    if nu == 2.0:
        assert len(set(piv)) < q  # a row is taken again: two noisy observations at one place
    P = piv
    A = Sig[np.ix_(P, P)] + nu * np.eye(q)
    closed = np.diag(Sig - Sig[:, P] @ np.linalg.solve(A, Sig[P, :]))
    assert np.allclose(resid, closed, rtol=0, atol=1e-12)
    Lf = np.tril(C[P], -1) + np.diag(np.sqrt(gain + nu))
    assert np.allclose(Lf @ Lf.T, A, rtol=0, atol=1e-12)
    assert np.allclose(C @ Lf.T, Sig[:, P], rtol=0, atol=1e-12)
    assert np.allclose(np.diag(C[P]) * np.sqrt(gain + nu), gain, rtol=0, atol=1e-13)
    assert np.all(resid > 0)


def test_restatement_stop_rule_on_a_duplicated_point():
    """A covariance whose last point is a copy of its first is singular: with nugget = 0 and
    tol = 0 the twin of a taken point is left with an exact 0 -- the rank is M - 1 -- while the
    M - 1 gains taken stay positive.  The entries are chosen so that the twin's arithmetic is
    exact (16 / sqrt(16), 16 - 4 * 4): nothing here depends on rounding."""
    Sig = np.diag([16.0, 9.0, 4.0, 1.0, 0.25, 16.0])
    Sig[0, 5] = Sig[5, 0] = 16.0
    Sig[1, 2] = Sig[2, 1] = 3.0
    M, k0 = 6, 16.0
    piv, C, resid, gain, rank = numpy_pivchol(Sig, k0, M)
    assert rank == M - 1
    assert list(piv) == [0, 1, 2, 3, 4, -1]  # of the twins the lower index is taken
    assert np.array_equal(gain, [16.0, 9.0, 3.0, 1.0, 0.25, 0.0])
    assert np.all(gain[:rank] > 0) and np.all(C[:, rank:] == 0.0)
    assert np.array_equal(C[5], [4.0, 0, 0, 0, 0, 0]) and np.all(resid == 0.0)
    assert np.allclose(C @ C.T, Sig, rtol=0, atol=1e-15)
    # a stop level between two gains ends there: at their geometric mean
    t = np.sqrt(gain[2] * gain[3]) / k0
    out = numpy_pivchol(Sig, k0, M, tol=t)
    assert out[4] == 3 and list(out[0]) == [0, 1, 2, -1, -1, -1]
    assert np.array_equal(out[3][3:], np.zeros(3)) and np.array_equal(out[2], [0, 0, 0, 1, 0.25, 0])
    # a nugget takes every step, the twins among them
    out = numpy_pivchol(Sig, k0, M, nugget=0.01)
    assert out[4] == M and np.all(out[2] > 0)


def test_restatement_tie_rule_and_non_finite_gains():
    Sig = np.diag([1.0, 2.0, 2.0, 0.5])
    piv, C, resid, gain, rank = numpy_pivchol(Sig, 1.0, 4)
    assert list(piv) == [1, 2, 0, 3] and rank == 4  # the lowest index among equals
    assert list(numpy_pivchol(np.eye(5), 1.0, 3)[0]) == [0, 1, 2]
    assert numpy_pivchol(np.diag([1.0, np.inf]), 1.0, 2)[4] == 0
    assert numpy_pivchol(np.diag([-1.0, -2.0]), 1.0, 2)[4] == 0
    assert numpy_pivchol(np.zeros((3, 3)), 1.0, 2)[4] == 0
    for bad in (dict(q=0), dict(q=5), dict(q=2, nugget=-1.0), dict(q=2, nugget=np.nan),
                dict(q=2, tol=-1e-3), dict(q=2, tol=np.inf)):
        with pytest.raises(ValueError):
            numpy_pivchol(Sig, 1.0, **bad)


# ---- the plumbing ----

def test_signature_is_declared():
    from bayesian_quadrature_amd import _lib
    import ctypes as C
    res, args = _lib.SIGNATURES["bq_gp_pivchol"]
    assert res is C.c_int and len(args) == 12
    assert args[3] is C.c_int64 and args[4] is C.c_int64
    assert args[5] is C.c_double and args[6] is C.c_double
    assert args[7] is _lib._i64p and args[11] is _lib._i64p


def test_gp_pivoted_cholesky_shapes_and_noisy(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.linspace(-2.9, 2.9, 17)
    piv, C, resid, gain = g.pivoted_cholesky(xo, 5)
    assert piv.shape == (5,) and piv.dtype == np.int64 and gain.shape == (5,)
    assert C.shape == (17, 5) and C.flags.f_contiguous and resid.shape == (17,)
    assert g._fit.calls[-1][1:5] == (17, 5, 0.0, 0.0)
    cov = np.asarray(g._fit.predict(xo, want_cov=True)[2])
    ref = numpy_pivchol(cov, kernel_scale(1.2, 0.8), 5)
    assert np.array_equal(piv, ref[0]) and np.array_equal(C, ref[1])
    assert np.array_equal(resid, ref[2]) and np.array_equal(gain, ref[3])
    # d x M points give the same
    again = g.pivoted_cholesky(xo[None, :], 5)
    assert all(np.array_equal(a, b) for a, b in zip(again, (piv, C, resid, gain)))
    # noisy: the nugget is s^2
    pn, Cn, rn, gn = g.pivoted_cholesky(xo, 5, noisy=True, tol=1e-9)
    assert g._fit.calls[-1][1:5] == (17, 5, 0.2 ** 2, 1e-9)
    refn = numpy_pivchol(cov, kernel_scale(1.2, 0.8), 5, nugget=0.2 ** 2, tol=1e-9)
    assert np.array_equal(pn, refn[0]) and np.array_equal(rn, refn[2]) and np.all(rn > 0)
    # a stop level above every gain: rank 0
    p0, C0, r0, g0 = g.pivoted_cholesky(xo, 5, tol=10.0)
    assert p0.shape == (0,) and C0.shape == (17, 0) and g0.shape == (0,)
    assert np.array_equal(r0, np.diag(cov))


def test_gp_greedy_design(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.linspace(-4.0, 4.0, 33)
    idx = g.greedy_design(xo, 6)
    assert g._fit.calls[-1][1:5] == (33, 6, 0.2 ** 2, 0.0)  # noisy by default
    assert idx.shape == (6,) and idx.dtype == np.int64
    assert np.array_equal(idx, g.pivoted_cholesky(xo, 6, noisy=True)[0])
    idx2, info = g.greedy_design(xo, 6, noisy=False, return_info=True)
    assert set(info) == {"gain", "resid"} and g._fit.calls[-1][3] == 0.0
    assert info["gain"].shape == (6,) and info["resid"].shape == (33,)
    assert np.all(info["resid"][idx2] == 0.0)
    # the design spreads: the six largest marginal variances crowd the two ends
    top = np.argsort(-g.var(xo))[:6]
    assert len(set(idx2.tolist())) == 6
    assert np.min(np.diff(np.sort(xo[idx2]))) > np.min(np.diff(np.sort(xo[top])))


def test_gp_pivoted_cholesky_empty_points_reach_no_device(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    g.pivoted_cholesky(np.array([0.1]), 1)
    n_calls = len(g._fit.calls)
    for xo in ([], np.empty(0), np.empty((1, 0))):
        piv, C, resid, gain = g.pivoted_cholesky(xo, 3)
        assert piv.shape == (0,) and piv.dtype == np.int64
        assert C.shape == (0, 0) and resid.shape == (0,) and gain.shape == (0,)
        idx, info = g.greedy_design(xo, 3, return_info=True)
        assert idx.shape == (0,) and info["gain"].shape == (0,) and info["resid"].shape == (0,)
    assert len(g._fit.calls) == n_calls


def test_gp_pivoted_cholesky_argument_errors(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.array([0.1, 0.5, -2.0])
    for fn in (g.pivoted_cholesky, g.greedy_design):
        for q in (0, -1, 4):
            with pytest.raises(ValueError):
                fn(xo, q)
        for tol in (-1e-3, np.nan, np.inf):
            with pytest.raises(ValueError):
                fn(xo, 2, tol=tol)
        with pytest.raises(ValueError):
            fn(np.zeros((2, 3)), 2)  # dimension mismatch
    assert g.pivoted_cholesky(xo, 3)[0].shape == (3,)


def test_gp_pivoted_cholesky_refits_pending_parameters_first(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.linspace(-2, 2, 9)
    a = g.pivoted_cholesky(xo, 4)
    fit = g._fit
    g.set_param("h", 1.3)
    b = g.pivoted_cholesky(xo, 4)
    assert g._fit is fit and fit.calls[-1][5] == 1.3
    assert not np.array_equal(a[3], b[3])


OPTIONS = {
    "n_candidate": 10, "x_mean": 0.0, "x_var": 10.0, "candidate_thresh": 0.5,
    "optim_method": "L-BFGS-B",
}


def test_bq_log_l_design(pkg):
    import scipy.stats
    np.random.seed(8728)
    x = np.linspace(-5, 5, 9)
    bq = pkg.BQ(x, scipy.stats.norm.pdf(x, 0, 1), kernel=pkg.GaussianKernel, **OPTIONS)
    bq.init(params_tl=(15, 2, 0.1), params_l=(0.2, 1.3, 0))
    x_c = np.linspace(-7, 7, 29)
    idx = bq.log_l_design(x_c, 4)
    assert idx.shape == (4,) and len(set(idx)) == 4
    assert np.array_equal(idx, bq.gp_log_l.greedy_design(x_c, 4))
    assert bq.gp_log_l._fit.calls[-1][1:4] == (29, 4, 0.1 ** 2)
    assert bq.log_l_design([], 4).shape == (0,)


def test_bq_log_l_design_raises_on_the_approximate_branch(pkg):
    import scipy.stats
    x = np.linspace(-3, 3, 5)
    bq = pkg.BQ(x, scipy.stats.norm.pdf(x, 0, 1), kernel=pkg.PeriodicKernel, **OPTIONS)
    assert bq.options["use_approx"]
    with pytest.raises(NotImplementedError):
        bq.log_l_design(np.array([0.1, 0.2]), 1)
