"""CPU tests of the polynomial trend of a fit with its coefficients marginalised: the contract of
bq_gp_trend / bq_gp_predict_trend restated in numpy (``numpy_trend``, in the precision of its
inputs), its properties checked on the restatement alone, and the host plumbing --
engine.Fit.trend / predict_trend's contract as gp.GP.trend, mean_trend, var_trend, log_lh_trend
and BQ.log_l_mean_trend / log_l_var_trend use it -- over the oracle-backed engine double with a
``trend`` / ``predict_trend`` built on the restatement.  test_gp_trend.py holds the device to the
same contract."""
import numpy as np
import pytest

from engine_double import EngineDouble, FitDouble
from test_gp_pivchol_host import OPTIONS, _data
from test_gp_sample import _case, _ld_gram

LD = np.longdouble
_LD_PI = LD(4) * np.arctan(LD(1))


def trend_p(degree, d):
    return (1, 1 + d, 1 + d + d * (d + 1) // 2)[degree]


def trend_basis(x, degree, c, rho):
    """H (m, p), rows phi(x_j)^T, for the points x (d, m) in their own precision: 1; t_1 .. t_d;
    t_k t_l for k <= l, k outer -- t = (x - c) / rho."""
    x = np.asarray(x)
    x = x[None, :] if x.ndim == 1 else x
    dt = x.dtype
    d = x.shape[0]
    t = (x - np.asarray(c, dtype=dt)[:, None]) / np.asarray(rho, dtype=dt)[:, None]
    cols = [np.ones(x.shape[1], dtype=dt)]
    if degree >= 1:
        cols += [t[k] for k in range(d)]
    if degree >= 2:
        cols += [t[k] * t[l] for k in range(d) for l in range(k, d)]
    return np.stack(cols, axis=1)


def default_basis(x):
    """The Python surface's default centre and scale for points x (d, n)."""
    x = np.asarray(x, dtype=np.float64)
    x = x[None, :] if x.ndim == 1 else x
    c = x.mean(axis=1)
    rho = np.max(np.abs(x - c[:, None]), axis=1)
    return c, np.where(rho > 0, rho, 1.0)


def chol(A):
    """Unblocked lower Cholesky factor in A's precision; LinAlgError at a pivot that is not
    positive and finite."""
    A = np.array(A)
    n = A.shape[0]
    Lf = np.zeros_like(A)
    for j in range(n):
        dj = A[j, j] - Lf[j, :j] @ Lf[j, :j]
        if not (dj > 0 and np.isfinite(dj)):
            raise np.linalg.LinAlgError("pivot %d is not positive and finite" % j)
        Lf[j, j] = np.sqrt(dj)
        Lf[j + 1:, j] = (A[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return Lf


def fwd(Lf, B):
    """L^-1 B by forward substitution in their precision."""
    X = np.array(B, dtype=Lf.dtype)
    for i in range(Lf.shape[0]):
        X[i] = (X[i] - Lf[i, :i] @ X[:i]) / Lf[i, i]
    return X


def bwd(Lf, B):
    """L^-T B by backward substitution."""
    X = np.array(B, dtype=Lf.dtype)
    for i in range(Lf.shape[0] - 1, -1, -1):
        X[i] = (X[i] - Lf[i + 1:, i] @ X[i + 1:]) / Lf[i, i]
    return X


def numpy_trend(Lf, z, H, V=None, Phi=None, k0=None, solve=fwd, solve_t=bwd):
    """The contract of bq_gp_trend, and with V (M, n; rows v_j = L^-1 k(x, xo_j)), Phi (M, p) and
    k0 = k(x, x) that of bq_gp_predict_trend, from the factor Lf of Kxx, z = L^-1 y and H, in their
    precision.  solve / solve_t: L^-1 B and L^-T B over the n x n factor (the tests' float64 route
    passes the oracle's); the p x p system is always solved here.  A dict: G, A, b, LA, beta,
    cov_beta, alpha_t, logml_t, btb and, with V, mean, var, R, quad (r_j^T A^-1 r_j)."""
    dt = Lf.dtype
    n, p = H.shape
    if n < p:
        raise ValueError("n < p")
    G = solve(Lf, H)
    A, b = G.T @ G, G.T @ z
    LA = chol(A)
    beta = bwd(LA, fwd(LA, b))
    W = fwd(LA, np.eye(p, dtype=dt))
    out = {"G": G, "A": A, "b": b, "LA": LA, "beta": beta, "cov_beta": W.T @ W}
    out["alpha_t"] = solve_t(Lf, z - G @ beta)
    out["btb"] = b @ beta
    two_pi = LD(2) * _LD_PI if dt == LD else 2 * np.pi
    out["logdet"] = 2 * np.sum(np.log(np.diag(Lf)))
    out["logdet_A"] = 2 * np.sum(np.log(np.diag(LA)))
    out["logml_t"] = (-(z @ z - out["btb"]) / 2 - out["logdet"] / 2 - out["logdet_A"] / 2
                      - (n - p) * np.log(two_pi) / 2)
    if V is not None:
        R = Phi - V @ G
        U = fwd(LA, R.T)
        out["R"], out["quad"] = R, np.sum(U * U, axis=0)
        out["mean"] = V @ z + R @ beta
        out["var"] = k0 - np.sum(V * V, axis=1) + out["quad"]
    return out


def ld_pieces(x, y, h, w, s, xo=None):
    """(Lf, z, V, k0) in long double for the Gaussian kernel of the library."""
    n = x.shape[1]
    Lf = chol(_ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD))
    z = fwd(Lf, y.astype(LD))
    V = None if xo is None else fwd(Lf, _ld_gram(x, xo, h, w)).T
    k0 = _ld_gram(x[:, :1], x[:, :1], h, w)[0, 0]
    return Lf, z, V, k0


def ld_trend(x, y, h, w, s, xo, degree, c=None, rho=None):
    """numpy_trend in long double for a problem, with the default basis unless one is given."""
    if c is None:
        c, rho = default_basis(x)
    Lf, z, V, k0 = ld_pieces(x, y, h, w, s, xo)
    H = trend_basis(x.astype(LD), degree, c, rho)
    Phi = None if xo is None else trend_basis(xo.astype(LD), degree, c, rho)
    out = numpy_trend(Lf, z, H, V, Phi, k0)
    out.update(Lf=Lf, z=z, V=V, k0=k0, H=H, Phi=Phi)
    return out


def scales(t):
    """The sizes the tests' bounds are relative to, from a numpy_trend dict with a prediction:
    (mean, var, beta (p,), logml_t)."""
    V, z, R, beta = t["V"], t["z"], t["R"], t["beta"]
    vn = np.sqrt(np.sum(V * V, axis=1))
    sm = np.max(vn * np.sqrt(z @ z) + np.abs(R) @ np.abs(beta))
    sv = t["k0"] + np.max(vn * vn) + np.max(t["quad"])
    sb = np.abs(t["cov_beta"]) @ np.abs(t["b"])
    sl = (z @ z + abs(t["btb"])) / 2 + abs(t["logdet"]) + abs(t["logdet_A"])
    return float(sm), float(sv), sb.astype(np.float64), float(sl)


class TrendFitDouble(FitDouble):
    """engine.Fit.trend / predict_trend over the oracle's Gram, factor and triangular solves."""

    def __init__(self, *args):
        self.calls = []
        FitDouble.__init__(self, *args)

    def _pts(self, a):
        a = np.asarray(a, dtype=np.float64)
        a = a[None, :] if a.ndim == 1 else a
        if a.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        return a

    def _key(self, degree, center, scale):
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        center = np.atleast_1d(np.asarray(center, dtype=np.float64)).ravel()
        scale = np.atleast_1d(np.asarray(scale, dtype=np.float64)).ravel()
        if center.shape != (self.d,) or scale.shape != (self.d,):
            raise ValueError("center and scale must have d entries")
        if degree not in (0, 1, 2):
            raise ValueError("trend: degree")
        if not np.all(np.isfinite(center)):
            raise ValueError("trend: the centre must be finite")
        if not (np.all(np.isfinite(scale)) and np.all(scale > 0)):
            raise ValueError("trend: the scale must be positive and finite")
        if self.n < trend_p(degree, self.d):
            raise ValueError("trend: fewer observations than basis functions")
        return int(degree), center, scale

    def _trend(self, degree, center, scale, xo=None):
        x = self._pts(self.x)
        H = trend_basis(x, degree, center, scale)
        V = Phi = k0 = None
        if xo is not None:
            V = self.o.trsm_lower(self._L, np.asfortranarray(self.o.gram_cross(x, xo, self.h,
                                                                                 self.w))).T
            Phi = trend_basis(xo, degree, center, scale)
            k0 = self.o.kernel_scale(self.d, self.h, self.w)
        return numpy_trend(np.asarray(self._L), self.z(), H, V, Phi, k0,
                           solve=lambda Lf, B: np.asarray(self.o.trsm_lower(Lf, B)),
                           solve_t=lambda Lf, B: np.linalg.solve(Lf.T, B))

    def trend(self, degree, center, scale):
        degree, center, scale = self._key(degree, center, scale)
        self.calls.append(("trend", degree, center.copy(), scale.copy(), self.h))
        t = self._trend(degree, center, scale)
        return t["beta"], np.asfortranarray(t["cov_beta"]), float(t["logml_t"]), t["alpha_t"]

    def predict_trend(self, xo, degree, center, scale, want_var=True):
        xo = self._pts(xo)
        degree, center, scale = self._key(degree, center, scale)
        self.calls.append(("predict_trend", degree, center.copy(), scale.copy(), self.h,
                           xo.shape[1], want_var))
        t = self._trend(degree, center, scale, xo)
        return t["mean"], (t["var"] if want_var else None)


class TrendEngineDouble(EngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return TrendFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def pkg(oracle):
    import bayesian_quadrature_amd as pkg
    from bayesian_quadrature_amd import engine as eng_mod
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(TrendEngineDouble(oracle), 0)
    yield pkg
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _np_problem(n=40, d=2, s=0.1, M=25, degree=2, seed=0):
    """A float64 problem and its restatement with plain numpy: (x, y, xo, c, rho, Lf, t)."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-3, 3, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    xo = rs.uniform(-4, 4, size=(d, M))
    w = np.full(d, 0.9)

    def k(a, b):
        q = sum((a[i][:, None] - b[i][None, :]) ** 2 / w[i] ** 2 for i in range(d))
        return 1.3 * np.exp(-0.5 * q)

    Lf = np.linalg.cholesky(k(x, x) + s * s * np.eye(n))
    c, rho = default_basis(x)
    H, Phi = trend_basis(x, degree, c, rho), trend_basis(xo, degree, c, rho)
    V = fwd(Lf, k(x, xo)).T
    return x, y, xo, H, Phi, Lf, V, 1.3


# ---- the restatement alone ----

@pytest.mark.parametrize("d,degree", [(1, 0), (1, 2), (2, 1), (2, 2), (3, 2)])
def test_restatement_alpha_is_orthogonal_to_the_basis(d, degree):
    x, y, xo, H, Phi, Lf, V, k0 = _np_problem(d=d, degree=degree)
    t = numpy_trend(Lf, fwd(Lf, y), H, V, Phi, k0)
    size = np.abs(H).T @ np.abs(t["alpha_t"])
    assert np.all(np.abs(H.T @ t["alpha_t"]) <= 1e-11 * size)
    # alpha_t is Kxx^-1 (y - H beta), and mean is k^T alpha_t + phi^T beta
    K = Lf @ Lf.T
    assert np.allclose(K @ t["alpha_t"], y - H @ t["beta"], rtol=0, atol=1e-10)
    assert np.allclose(t["mean"], (V @ Lf.T) @ t["alpha_t"] + Phi @ t["beta"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("d,degree", [(1, 2), (2, 1), (3, 2)])
def test_restatement_shift_of_the_targets_within_the_span(d, degree):
    x, y, xo, H, Phi, Lf, V, k0 = _np_problem(d=d, degree=degree)
    p = H.shape[1]
    gamma = np.random.RandomState(5).uniform(-2, 2, p)
    a = numpy_trend(Lf, fwd(Lf, y), H, V, Phi, k0)
    b = numpy_trend(Lf, fwd(Lf, y + H @ gamma), H, V, Phi, k0)
    assert np.allclose(b["beta"] - a["beta"], gamma, rtol=0, atol=1e-9)
    assert np.array_equal(b["var"], a["var"])
    assert abs(b["logml_t"] - a["logml_t"]) <= 1e-9 * abs(a["logml_t"])
    assert np.allclose(b["mean"] - a["mean"], Phi @ gamma, rtol=0, atol=1e-8)
    assert np.allclose(b["alpha_t"], a["alpha_t"], rtol=0, atol=1e-8)


@pytest.mark.parametrize("d,degree", [(1, 0), (1, 2), (2, 2), (3, 1)])
def test_restatement_variance_is_not_below_the_zero_mean_one(d, degree):
    x, y, xo, H, Phi, Lf, V, k0 = _np_problem(d=d, degree=degree)
    t = numpy_trend(Lf, fwd(Lf, y), H, V, Phi, k0)
    assert np.all(t["quad"] >= 0) and np.all(t["var"] >= k0 - np.sum(V * V, axis=1))
    assert np.max(t["quad"]) > 1e-3 * k0
    assert np.allclose(t["cov_beta"] @ t["A"], np.eye(H.shape[1]), rtol=0, atol=1e-10)


def _quadratic_example():
    """The issue's example: log l = -(x - 0.4)^2 / (2 0.7^2) - 1.3 at 13 points on [-3, 3], h = 2,
    w = 1, s = 1e-3, queried at x = 6.  (Lf, z, y, V, k0, x, xo) in float64."""
    x = np.linspace(-3, 3, 13)
    y = -(x - 0.4) ** 2 / (2 * 0.7 ** 2) - 1.3
    xo = np.array([6.0])

    def k(a, b):
        return 4.0 / np.sqrt(2 * np.pi) * np.exp(-0.5 * (a[:, None] - b[None, :]) ** 2)

    Lf = np.linalg.cholesky(k(x, x) + 1e-6 * np.eye(13))
    return Lf, fwd(Lf, y), y, fwd(Lf, k(x, xo)).T, 4.0 / np.sqrt(2 * np.pi), x, xo


def test_restatement_reproduces_targets_in_the_span_outside_the_data():
    Lf, z, y, V, k0, x, xo = _quadratic_example()
    c, rho = default_basis(x)
    t = numpy_trend(Lf, z, trend_basis(x, 2, c, rho), V, trend_basis(xo, 2, c, rho), k0)
    truth = -(6.0 - 0.4) ** 2 / (2 * 0.7 ** 2) - 1.3
    zero_mean = float(V[0] @ z)
    print("x = 6: truth %.4f, zero-mean %.4f, trend %.6f; var %.4f against %.4f"
          % (truth, zero_mean, t["mean"][0], t["var"][0], k0 - V[0] @ V[0]))
    assert abs(truth - (-33.3)) < 0.01 and zero_mean > -1.0
    assert abs(t["mean"][0] - truth) < 1e-3
    assert abs(t["var"][0] - 13.3) < 0.1 and abs((k0 - V[0] @ V[0]) - 1.59) < 0.01
    # every target in the span, any degree-2 polynomial, any query point
    rs = np.random.RandomState(2)
    xq = rs.uniform(-9, 9, 7)
    for co in rs.uniform(-2, 2, (3, 3)):
        yy = co[0] + co[1] * x + co[2] * x * x
        Vq = fwd(Lf, 4.0 / np.sqrt(2 * np.pi) * np.exp(-0.5 * (x[:, None] - xq[None, :]) ** 2)).T
        tt = numpy_trend(Lf, fwd(Lf, yy), trend_basis(x, 2, c, rho), Vq,
                         trend_basis(xq, 2, c, rho), k0)
        want = co[0] + co[1] * xq + co[2] * xq * xq
        assert np.allclose(tt["mean"], want, rtol=0, atol=1e-6 * np.max(np.abs(want)))
        assert np.allclose(tt["alpha_t"], 0, rtol=0, atol=1e-5)


@pytest.mark.parametrize("n,d,degree", [(65, 1, 2), (130, 3, 2), (65, 3, 1)])
def test_restatement_is_the_limit_of_a_vague_prior_on_the_coefficients(n, d, degree):
    """A zero-mean GP with kernel k + b^2 phi phi^T approaches mean_t and var_t like 1 / b^2, in
    long double: the distance at b^2 = 1e4 is between 50 and 200 times that at 1e6, which is below
    1e-7 of the scales."""
    x, y, h, w, s, xo = _case(n, d, 0.1, 20, 1.0)
    t = ld_trend(x, y, h, w, s, xo, degree)
    sm, sv, _, _ = scales(t)
    Kxx = t["Lf"] @ t["Lf"].T
    Kxo = t["Lf"] @ t["V"].T
    H, Phi = t["H"], t["Phi"]
    dist = {}
    for b2 in (LD(1e4), LD(1e6)):
        Lb = chol(Kxx + b2 * (H @ H.T))
        Vb = fwd(Lb, Kxo + b2 * (H @ Phi.T)).T
        mean_b = Vb @ fwd(Lb, y.astype(LD))
        var_b = t["k0"] + b2 * np.sum(Phi * Phi, axis=1) - np.sum(Vb * Vb, axis=1)
        dist[float(b2)] = (float(np.max(np.abs(mean_b - t["mean"]))) / sm,
                           float(np.max(np.abs(var_b - t["var"]))) / sv)
    print("n=%d d=%d degree=%d: distance / scale %s" % (n, d, degree, dist))
    for q in (0, 1):
        assert dist[1e6][q] < 1e-7
        assert 50 <= dist[1e4][q] / dist[1e6][q] <= 200


def test_restatement_basis_order_and_argument_rules():
    x = np.array([[1.0, 2.0], [3.0, 5.0], [-1.0, 0.5]])
    c, rho = np.array([1.0, 1.0, 0.0]), np.array([2.0, 4.0, 0.5])
    t = (x - c[:, None]) / rho[:, None]
    H = trend_basis(x, 2, c, rho)
    want = [np.ones(2), t[0], t[1], t[2], t[0] * t[0], t[0] * t[1], t[0] * t[2], t[1] * t[1],
            t[1] * t[2], t[2] * t[2]]
    assert H.shape == (2, 10) and np.array_equal(H, np.stack(want, axis=1))
    assert np.array_equal(trend_basis(x, 1, c, rho), H[:, :4])
    assert np.array_equal(trend_basis(x, 0, c, rho), H[:, :1])
    assert [trend_p(g, 8) for g in (0, 1, 2)] == [1, 9, 45]
    assert trend_basis(np.array([0.5, 1.5]), 2, [0.5], [2.0]).shape == (2, 3)
    cc, rr = default_basis(np.array([[0.0, 2.0, 4.0], [7.0, 7.0, 7.0]]))
    assert np.array_equal(cc, [2.0, 7.0]) and np.array_equal(rr, [2.0, 1.0])
    with pytest.raises(ValueError):  # n < p
        numpy_trend(np.eye(2), np.ones(2), np.ones((2, 3)))
    with pytest.raises(np.linalg.LinAlgError):  # coincident points: H has rank 1
        numpy_trend(np.eye(4), np.ones(4), np.ones((4, 3)))


# ---- the plumbing ----

def test_signatures_are_declared():
    from bayesian_quadrature_amd import _lib
    import ctypes as C
    res, args = _lib.SIGNATURES["bq_gp_trend"]
    assert res is C.c_int and len(args) == 9
    assert args[0] is C.c_void_p and args[1] is C.c_void_p and args[2] is C.c_int
    assert all(a is _lib._dp for a in args[3:])
    res, args = _lib.SIGNATURES["bq_gp_predict_trend"]
    assert res is C.c_int and len(args) == 9
    assert args[0] is C.c_void_p and args[1] is C.c_void_p and args[2] is C.c_int
    assert all(args[i] is _lib._dp for i in (3, 4, 5, 7, 8)) and args[6] is C.c_int64


def test_fit_trend_argument_errors(pkg, oracle):
    x, y = _data(n=12)
    fit = TrendFitDouble(oracle, x, y, 1.2, 0.8, 0.2)
    c, rho = default_basis(x)
    assert fit.trend(2, c, rho)[0].shape == (3,)
    for degree in (-1, 3):
        with pytest.raises(ValueError):
            fit.trend(degree, c, rho)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            fit.trend(2, [bad], rho)
        with pytest.raises(ValueError):
            fit.predict_trend(x, 2, c, [bad])
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            fit.trend(1, c, [bad])
    with pytest.raises(ValueError):  # d entries each
        fit.trend(1, [0.0, 0.0], rho)
    with pytest.raises(ValueError):  # n < p
        TrendFitDouble(oracle, x[:2], y[:2], 1.2, 0.8, 0.2).trend(2, c, rho)
    assert TrendFitDouble(oracle, x[:3], y[:3], 1.2, 0.8, 0.2).trend(2, c, rho)[0].shape == (3,)
    with pytest.raises(ValueError):  # dimension mismatch of the query points
        fit.predict_trend(np.zeros((2, 3)), 1, c, rho)
    # n >= p coincident points: H^T Kxx^-1 H is singular
    xx = np.zeros((2, 6)) + np.array([[0.3], [-0.2]])
    with pytest.raises(np.linalg.LinAlgError):
        TrendFitDouble(oracle, xx, np.arange(6.0), 1.2, np.array([0.8, 0.8]), 0.1).trend(
            2, [0.3, -0.2], [1.0, 1.0])


def test_gp_trend_defaults_and_values(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    beta, cov, logml, alpha = g.trend()
    call = g._fit.calls[-1]
    c, rho = float(np.mean(x)), float(np.max(np.abs(x - np.mean(x))))
    assert call[:2] == ("trend", 2) and np.array_equal(call[2], [c]) and np.array_equal(call[3], [rho])
    assert beta.shape == (3,) and cov.shape == (3, 3) and alpha.shape == (40,)
    assert isinstance(logml, float) and g.log_lh_trend() == logml
    assert np.allclose(cov, cov.T, rtol=0, atol=1e-14) and np.all(np.linalg.eigvalsh(cov) > 0)
    assert g.trend(0)[0].shape == (1,) and g.trend(1)[0].shape == (2,)
    assert g.log_lh_trend(1) == g.trend(1)[2] != logml
    xo = np.linspace(-5, 5, 11)
    m, v = g.mean_var_trend(xo)
    assert g._fit.calls[-1][:2] == ("predict_trend", 2) and g._fit.calls[-1][5:] == (11, True)
    m1 = g.mean_trend(xo)
    assert g._fit.calls[-1][6] is False
    assert np.array_equal(m, m1) and np.array_equal(g.var_trend(xo), v)
    assert np.all(v >= g.var(xo) - 1e-13) and np.max(v - g.var(xo)) > 1e-2
    # the mean is k^T alpha_t + phi^T beta with the memoised trend
    phi = trend_basis(xo, 2, [c], [rho])
    assert np.allclose(m, g.Kxox(xo) @ alpha + phi @ beta, rtol=0, atol=1e-10)
    # the zero-mean surface is untouched
    assert g.log_lh != logml and np.max(np.abs(g.mean(xo) - m)) > 1e-3
    # a constant x: scale 1
    g2 = pkg.GP(pkg.GaussianKernel(1.2, 0.8), np.array([0.5]), np.array([1.0]), s=0.2)
    assert g2.trend(0)[0].shape == (1,)
    assert np.array_equal(g2._fit.calls[-1][2], [0.5]) and np.array_equal(g2._fit.calls[-1][3], [1.0])
    for degree in (-1, 3, 1.5, "2", True):
        with pytest.raises(ValueError):
            g.trend(degree)
        with pytest.raises(ValueError):
            g.mean_trend(xo, degree)
    for empty in ([], np.empty(0)):
        n_calls = len(g._fit.calls)
        assert g.mean_trend(empty).shape == (0,) and g.var_trend(empty).shape == (0,)
        assert len(g._fit.calls) == n_calls


def test_gp_trend_is_memoised_and_invalidated(pkg):
    x, y = _data()
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    a = g.trend()
    n_calls = len(g._fit.calls)
    assert g.trend() is a and g.log_lh_trend() == a[2] and len(g._fit.calls) == n_calls
    assert g.trend(1) is not a and g.trend(1) is g.trend(1)

    def fresh(what):
        b = g.trend()
        assert b is not a, what
        assert g._fit.calls[-1][0] == "trend"
        return b

    g.set_param("h", 1.3)
    b = fresh("h")
    assert g._fit.calls[-1][4] == 1.3 and not np.array_equal(a[0], b[0])
    g.s = 0.25
    c = fresh("s")
    g.y = y + 1.0
    e = fresh("y")
    assert np.allclose(e[0][0] - c[0][0], 1.0, rtol=0, atol=1e-9)  # a shift within the span
    g.x = x + 0.5  # the centre moves with the data
    fresh("x")
    assert np.array_equal(g._fit.calls[-1][2], [float(np.mean(x + 0.5))])
    g.append(np.array([3.5]), np.array([0.2]))
    f = fresh("append")
    assert f[3].shape == (41,)
    assert np.array_equal(g._fit.calls[-1][2], [float(np.mean(g.x))])
    assert np.array_equal(g._fit.calls[-1][3], [float(np.max(np.abs(g.x - np.mean(g.x))))])
    g.remove([0, 5])
    assert fresh("remove")[3].shape == (39,)


def test_bq_log_l_trend(pkg):
    import scipy.stats
    np.random.seed(8728)
    x = np.linspace(-5, 5, 9)
    bq = pkg.BQ(x, scipy.stats.norm.pdf(x, 0, 1), kernel=pkg.GaussianKernel, **OPTIONS)
    bq.init(params_tl=(15, 2, 0.1), params_l=(0.2, 1.3, 0))
    xq = np.array([-8.0, 0.3, 8.0])
    m = bq.log_l_mean_trend(xq)
    assert bq.gp_log_l._fit.calls[-1][:2] == ("predict_trend", 2)
    v = bq.log_l_var_trend(xq)
    assert np.array_equal(m, bq.gp_log_l.mean_trend(xq))
    assert np.array_equal(v, bq.gp_log_l.var_trend(xq))
    # log N(x | 0, 1) is a quadratic: the trend follows it out of the samples' range
    truth = scipy.stats.norm.logpdf(xq, 0, 1)
    assert np.max(np.abs(m - truth)) < 0.05 * np.max(np.abs(truth))
    assert np.max(np.abs(bq.gp_log_l.mean(xq) - truth)) > 10 * np.max(np.abs(m - truth))
    assert np.array_equal(bq.log_l_mean_trend(xq, degree=1), bq.gp_log_l.mean_trend(xq, 1))
    assert bq.gp_log_l._fit.calls[-1][1] == 1


def test_bq_log_l_trend_raises_on_the_approximate_branch(pkg):
    import scipy.stats
    x = np.linspace(-3, 3, 5)
    bq = pkg.BQ(x, scipy.stats.norm.pdf(x, 0, 1), kernel=pkg.PeriodicKernel, **OPTIONS)
    assert bq.options["use_approx"]
    with pytest.raises(NotImplementedError):
        bq.log_l_mean_trend(np.array([0.1, 0.2]))
    with pytest.raises(NotImplementedError):
        bq.log_l_var_trend(np.array([0.1, 0.2]))
