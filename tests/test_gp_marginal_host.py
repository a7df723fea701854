"""CPU tests of the marginal of a fit: ld_marginal.py's references held to independent derivations
(mpmath quadrature over the integrated axes, d = 2 and d = 3, both kinds of measure), the two
identities that tie a marginal to ``integral`` -- its integral over q is Z, the double integral of
its covariance is var Z -- on a fit double in float64, a demonstration on a correlated bump, and
the host plumbing (gp.GP.marginal's memo, the shapes, the errors) over that double, which extends
test_gp_measures_host.MeasureFitDouble with the float64 yardsticks of ld_marginal.py.
test_gp_marginal.py holds the device to the same references."""
import mpmath
import numpy as np
import pytest

import ld_marginal as lm
from ld_closed_forms import EPS, MARGIN, all_normal
from test_gp_measures_host import MeasureEngineDouble, MeasureFitDouble


def _ms():
    from bayesian_quadrature_amd import measures
    return measures


class MargFitDouble(MeasureFitDouble):
    """MeasureFitDouble with engine.Fit.marginal's signature: c and P from ld_marginal's float64
    yardsticks, the posterior by the contract's algebra in numpy."""

    def marginal(self, xq, axes, mu, cov=None, want_mean=True, want_var=True, want_cov=False):
        from bayesian_quadrature_amd.engine import _marginal_no_mixture, _marginal_points
        _marginal_no_mixture(mu)
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        keep, full = _marginal_points(xq, axes, self.d)
        if not 0 < keep.sum() < self.d:
            raise ValueError("a marginal keeps between 1 and d - 1 axes")
        S = sorted(int(a) for a in np.flatnonzero(keep))
        q = full[S]
        if not np.all(np.isfinite(q)):
            raise ValueError("a kept coordinate of a query point is not finite")
        self.calls.append(("marginal", tuple(S), q.shape[1], want_cov, self.h))
        if isinstance(mu, _ms().Measure):
            if cov is not None:
                raise TypeError("a measure object comes without a cov")
            c, P = lm.f64_marg_box(q, self.x, self.h, self.w, S, mu.lo, mu.hi)
        else:
            mu, cov = self._measure(mu, cov)
            c, P = lm.f64_marg_gauss(q, self.x, self.h, self.w, S, mu, cov)
        L = np.linalg.cholesky(np.asarray(self.K()))
        V = np.linalg.solve(L, c.T).T
        z = np.linalg.solve(L, self.y)
        Sig = P - V @ V.T
        return (V @ z if want_mean else None, np.diag(Sig).copy() if want_var else None,
                Sig if want_cov else None)


class MargEngineDouble(MeasureEngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return MargFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def pkg(oracle):
    import bayesian_quadrature_amd as pkg
    from bayesian_quadrature_amd import engine as eng_mod
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(MargEngineDouble(oracle), 0)
    yield pkg
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


# ---- the references and the yardsticks ----

@pytest.mark.parametrize("d", lm.DIMS)
def test_references_are_normal_and_the_yardsticks_error(d):
    """r per family (CPU, in eps: Gaussian 2 .. 40 for the cross matrix and the prior, the largest
    at flat, d = 8; box about 2) -- recorded, and every reference entry a normal number."""
    for axes in lm.keep_sets(d):
        for fam in lm.GAUSS_FAMILIES:
            c = lm.gauss_case(fam, d, axes)
            assert all_normal(c["ref"]) and all_normal(c["P"]) and c["live"].all()
            print("gauss %s d=%d keep %s: r %.1f eps, r_p %.1f eps, smallest entry %.3g"
                  % (fam, d, axes, c["r"] / EPS, c["r_p"] / EPS, float(c["ref"].min())))
            assert np.isfinite(c["r"]) and np.isfinite(c["r_p"])
        c = lm.box_case(d, axes)
        assert all_normal(c["ref"]) and all_normal(c["pdiag"])
        print("box d=%d keep %s: r %.1f eps, r_p %.1f eps" % (d, axes, c["r"] / EPS, c["r_p"] / EPS))
    # the far pair of the Gaussian families reaches past 1e-180 and is still normal
    assert float(lm.gauss_case("tight", d, lm.keep_sets(d)[-1])["ref"].min()) < 1e-150


def _mp(v):
    return mpmath.mpf(float(v))


def _mp_gauss_density(mu, cov):
    """p -> N(p | mu, cov) for mpmath vectors, through the explicit inverse."""
    k = len(mu)
    C = mpmath.matrix(k, k)
    for r in range(k):
        for c in range(k):
            C[r, c] = _mp(cov[r, c])
    Ci, norm = mpmath.inverse(C), mpmath.sqrt((2 * mpmath.pi) ** k * mpmath.det(C))

    def dens(p):
        z = [p[r] - _mp(mu[r]) for r in range(k)]
        return mpmath.exp(-sum(z[r] * Ci[r, c] * z[c] for r in range(k) for c in range(k)) / 2) \
            / norm
    return dens


def _mp_kernel(a, b, h, w):
    v = _mp(h) ** 2
    for k in range(len(w)):
        v *= mpmath.npdf(a[k], b[k], _mp(w[k]))
    return v


def _full(d, S, q, t):
    I = [k for k in range(d) if k not in S]
    p = [None] * d
    for a, k in enumerate(S):
        p[k] = q[a]
    for a, k in enumerate(I):
        p[k] = t[a]
    return p


HOST_CASES = [(2, (0,)), (2, (1,)), (3, (0, 2)), (3, (0, 1))]


@pytest.mark.parametrize("d,axes", HOST_CASES)
@pytest.mark.parametrize("kind", ("gauss", "box"))
def test_references_against_quadrature(kind, d, axes):
    """c(q, x) = int k((q, t), x) pi(q, t) dt by mpmath.quad over the integrated axes, and -- with
    one integrated axis -- P(q, q') = int int k((q, t), (q', t')) pi(q, t) pi(q', t') dt dt', at
    20 digits in pieces about the measure; the closed forms agree to 1e-15."""
    S, I = lm.split(d, axes)
    w = lm.lengths(d)
    rs = np.random.RandomState(5 + d + len(S))
    x = rs.uniform(-1.0, 1.5, (d, 2))
    xq = rs.uniform(-1.0, 1.5, (len(S), 2))
    if kind == "gauss":
        mu = 0.4 * np.where(np.arange(d) % 2 == 0, 1.0, -0.5)
        cov = 1.2 ** 2 * ((1 - 0.3) * np.eye(d) + 0.3)
        ref, Pref = lm.ld_marg_gauss(xq, x, lm.H, w, axes, mu, cov)
        cuts = [mpmath.mpf(v) for v in (-12, -6, -3, -1, 1, 3, 6, 12)]
    else:
        lo, hi = np.full(d, -2.0), np.full(d, 3.0)
        ref, Pref = lm.ld_marg_box(xq, x, lm.H, w, axes, lo, hi)
        cuts = [mpmath.mpf(v) for v in (-2, -1, 0, 1, 2, 3)]

        def dens(p):
            return mpmath.mpf(1) / mpmath.mpf(5) ** d
    with mpmath.workdps(20):
        if kind == "gauss":
            dens = _mp_gauss_density(mu, cov)
        for i in range(2):
            q = [_mp(v) for v in xq[:, i]]
            xj = [_mp(v) for v in x[:, 0]]

            def f(*t):
                p = _full(d, S, q, t)
                return _mp_kernel(p, xj, lm.H, w) * dens(p)
            got = mpmath.quad(f, *([cuts] * len(I)), method="gauss-legendre")
            err = abs(mpmath.mpf(str(ref[i, 0])) / got - 1)
            print("%s d=%d keep %s: c against quadrature %s" % (kind, d, axes, mpmath.nstr(err, 3)))
            assert err < 1e-15
        if len(I) == 1:
            qa, qb = ([_mp(v) for v in xq[:, i]] for i in range(2))

            def g(t, u):
                pa, pb = _full(d, S, qa, [t]), _full(d, S, qb, [u])
                return _mp_kernel(pa, pb, lm.H, w) * dens(pa) * dens(pb)
            got = mpmath.quad(g, cuts, cuts, method="gauss-legendre")
            err = abs(mpmath.mpf(str(Pref[0, 1])) / got - 1)
            print("%s d=%d keep %s: P against quadrature %s" % (kind, d, axes, mpmath.nstr(err, 3)))
            assert err < 1e-12


# ---- the two identities ----

def _bump_fit(pkg, n=40, seed=2):
    """A correlated two-dimensional Gaussian bump at n points and the prior N(0, Sigma), rho != 0."""
    rs = np.random.RandomState(seed)
    x = np.asfortranarray(rs.uniform(-2.5, 2.5, (2, n)))
    A = np.linalg.inv(np.array([[0.8, 0.35], [0.35, 0.6]]))
    y = np.exp(-0.5 * np.einsum("in,ij,jn->n", x - 0.3, A, x - 0.3))
    from bayesian_quadrature_amd import get_engine
    fit = get_engine(0).gp_fit(x, y, 0.9, np.array([0.8, 0.7]), 1e-3)
    return fit, x, y, A


def _legendre(a, b, G):
    t, wt = np.polynomial.legendre.leggauss(G)
    return 0.5 * (b - a) * t + 0.5 * (a + b), 0.5 * (b - a) * wt


@pytest.mark.parametrize("kind", ("gauss", "box"))
def test_marginal_integrates_to_the_integral(pkg, kind):
    """int J(q) dq = Z and int int cov(q, q') dq dq' = var Z, d = 2, keep axis 0, by a
    Gauss-Legendre rule over q -- the box's own side, or 9 standard deviations of the Gaussian
    about its mean (tail mass 2e-19).  The tolerance is the rule's own error, G against 2 G nodes
    on the same function, plus MARGIN 4 eps of the scale (observed at G = 96: quadrature error
    4.8e-15 / 2.9e-17 (Gaussian: Z 0.3313, var Z 9.896e-4) and 2.4e-15 / 7.4e-17 (box: 0.2367,
    2.841e-3); the identities are off by 0.003 .. 0.38 of their tolerances)."""
    fit, x, y, A = _bump_fit(pkg)
    if kind == "box":
        meas, a, b = (_ms().BoxMeasure([-2.0, -1.5], [2.5, 2.0]),), -2.0, 2.5
    else:
        cov = np.array([[1.0, 0.45], [0.45, 1.4]])
        meas, a, b = (np.array([0.1, -0.2]), cov), 0.1 - 9.0, 0.1 + 9.0
    Z, varZ = fit.integral(*meas)

    def rule(G):
        q, wt = _legendre(a, b, G)
        mean, _, cv = fit.marginal(q, [0], *meas, want_cov=True)
        return wt @ mean, wt @ cv @ wt, wt @ np.abs(mean), wt @ np.abs(cv) @ wt

    G = 96
    zm, zv, sm, sv = rule(G)
    zm2, zv2, _, _ = rule(2 * G)
    tol_m = abs(zm - zm2) + MARGIN * 4 * EPS * sm
    tol_v = abs(zv - zv2) + MARGIN * 4 * EPS * sv
    print("%s: Z %.6g, rule %.6g, quadrature error %.3g; var Z %.6g, rule %.6g, quadrature error "
          "%.3g; identities off by %.3g and %.3g of their tolerances"
          % (kind, Z, zm, abs(zm - zm2), varZ, zv, abs(zv - zv2), abs(zm - Z) / tol_m,
             abs(zv - varZ) / tol_v))
    assert abs(zm - Z) <= tol_m and abs(zv - varZ) <= tol_v


# ---- a demonstration ----

def test_demonstration_marginal_of_a_correlated_bump(pkg):
    """f a correlated bump at 40 points, pi = N(0, Sigma) with rho = 0.4: the marginal over axis
    1 contains the closed-form marginal of f pi within three of its own standard deviations at
    every plot point, J / Z integrates to 1, and the route a user takes today -- predict on a
    16-node Gauss-Hermite grid per plot point -- gives the same mean and no variance.
    (Observed: the largest |J - truth| / sd over 41 plot points 0.38, sd between 0.6 % and 10 % of
    max J; int J / Z - 1 = -7e-15; the Gauss-Hermite mean within 2.6e-4 of max J, 16 predictions
    per plot point.)"""
    fit, x, y, A = _bump_fit(pkg)
    Sig = np.array([[1.0, 0.4], [0.4, 1.3]])
    mu = np.zeros(2)
    q = np.linspace(-2.0, 2.5, 41)
    mean, var, _ = fit.marginal(q, [0], mu, Sig)
    # f pi = exp(-(x - c)' A (x - c) / 2) N(x | 0, Sig): a Gaussian in x, integrated over x_1
    Pi = np.linalg.inv(Sig)
    Lam = A + Pi
    c = np.full(2, 0.3)
    m = np.linalg.solve(Lam, A @ c)
    const = np.exp(-0.5 * (c @ A @ c - m @ Lam @ m)) / (2 * np.pi * np.sqrt(np.linalg.det(Sig)))
    C = np.linalg.inv(Lam)
    truth = const * np.sqrt(2 * np.pi * np.linalg.det(C) / C[0, 0]) * \
        np.exp(-0.5 * (q - m[0]) ** 2 / C[0, 0])
    sd = np.sqrt(np.maximum(var, 0.0))
    print("largest |J - truth| / sd %.3g; sd / max J between %.3g and %.3g"
          % (np.max(np.abs(mean - truth) / sd), sd.min() / mean.max(), sd.max() / mean.max()))
    assert np.all(np.abs(mean - truth) <= 3.0 * sd)
    # J / Z integrates to 1
    Z = fit.integral(mu, Sig)[0]
    g, wt = _legendre(-9.0, 9.0, 192)
    total = wt @ fit.marginal(g, [0], mu, Sig, want_var=False)[0] / Z
    print("int J / Z - 1 = %.3g" % (total - 1.0))
    assert abs(total - 1.0) <= 1e-12
    # the naive route: the conditional of x_1 given q by Gauss-Hermite, times pi_S(q)
    t, wh = np.polynomial.hermite_e.hermegauss(16)
    wh = wh / np.sqrt(2 * np.pi)
    Bc, sc = Sig[1, 0] / Sig[0, 0], np.sqrt(Sig[1, 1] - Sig[1, 0] ** 2 / Sig[0, 0])
    piS = np.exp(-0.5 * q ** 2 / Sig[0, 0]) / np.sqrt(2 * np.pi * Sig[0, 0])
    naive = np.array([piS[i] * (wh @ fit.predict(
        np.vstack([np.full(16, q[i]), Bc * q[i] + sc * t]), want_var=False)[0])
        for i in range(len(q))])
    print("Gauss-Hermite mean against marginal: %.3g of max J" % (
        np.max(np.abs(naive - mean)) / mean.max()))
    # (a 16-node rule is exact to degree 31 of the standard normal; the integrand is a sum of
    # bumps of width a = w_1 / sc in its variable, for which the rule's error falls like
    # (1 + a^2)^-16: the bound, of the largest value)
    assert np.max(np.abs(naive - mean)) <= (1.0 + (0.7 / sc) ** 2) ** -16 * mean.max()


# ---- host plumbing ----

def test_gp_marginal_memo_shapes_and_errors(pkg):
    fit, x, y, A = _bump_fit(pkg)
    mu, Sig = np.zeros(2), np.array([[1.0, 0.4], [0.4, 1.3]])
    q = np.linspace(-1.0, 1.0, 5)
    a = fit.marginal(q, [1], mu, Sig)
    b = fit.marginal(q[None, :], (1,), mu, Sig)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] is None
    assert fit.marginal(q, [0], mu, Sig, want_mean=False, want_var=False, want_cov=True)[2].shape \
        == (5, 5)
    for bad in ([], [0, 1], [2], [0, 0], [-1]):
        with pytest.raises(ValueError):
            fit.marginal(np.zeros((len(bad), 3)), bad, mu, Sig)
    with pytest.raises(ValueError):
        fit.marginal(np.zeros((2, 3)), [0], mu, Sig)              # two rows for one axis
    with pytest.raises(ValueError):
        fit.marginal(np.array([0.0, np.nan]), [0], mu, Sig)
    mix = _ms().GaussianMixture([1.0], [[0.0, 0.0]], [np.eye(2)])
    with pytest.raises(ValueError, match="mixture"):
        fit.marginal(q, [0], mix)
    with pytest.raises(TypeError):
        fit.marginal(q, [0], _ms().BoxMeasure([-1.0, -1.0], [1.0, 1.0]), Sig)

    # gp.GP is one-dimensional: it has no marginal, and says so through the fit
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), np.linspace(-2, 2, 9), np.sin(np.linspace(-2, 2, 9)),
               s=0.1)
    with pytest.raises(ValueError):
        g.marginal([0], q, 0.0, 1.0)
    with pytest.raises(ValueError, match="mixture"):
        g.marginal([0], q, _ms().GaussianMixture([1.0], [[0.0]], [[[1.0]]]))
    # the memo and its invalidation, over a GP whose resident fit is the two-dimensional double
    g._fit, g._fit_params = fit, (g.K.h, g.K.w, g._s)
    g._x = x
    n0 = len(fit.calls)
    m1 = g.marginal([0], q, mu, Sig)
    assert len(fit.calls) == n0 + 1 and fit.calls[-1][0] == "marginal"
    m2 = g.marginal((0,), q.copy(), mu.copy(), Sig.copy())
    assert len(fit.calls) == n0 + 1 and all(np.array_equal(u, v) for u, v in zip(m1, m2))
    m1[0][:] = 0.0                                                # a copy leaves: the memo stays
    assert np.array_equal(g.marginal([0], q, mu, Sig)[0], m2[0])
    cv = g.marginal_cov([0], q, mu, Sig)
    assert len(fit.calls) == n0 + 2 and cv.shape == (5, 5)
    assert np.allclose(np.diag(cv), m2[1], rtol=0, atol=1e-14)
    g.marginal([1], q, mu, Sig), g.marginal([0], q + 0.5, mu, Sig), g.marginal([0], q, mu, 2 * Sig)
    assert len(fit.calls) == n0 + 5
    g.integral(mu, Sig)
    g._invalidate(data_changed=False)                             # what drops integral's memo
    g._fit_params = (g.K.h, g.K.w, g._s)                          # (no refit of the planted fit)
    n1 = len(fit.calls)
    g.marginal([0], q, mu, Sig), g.integral(mu, Sig)
    assert len(fit.calls) == n1 + 2


def test_marginal_is_the_only_view_outside_the_table():
    """Every public name of engine.Fit is its own -- a row of test_gp_fit_state.ROWS or one of its
    NOT_CONSUMERS, as that file's test holds -- or ``marginal``, whose rows are test_gp_marginal.MROWS: no other
    consumer may come in through the base class."""
    from bayesian_quadrature_amd import engine as eng_mod
    public = {k for k in dir(eng_mod.Fit) if not k.startswith("_")
              and (callable(getattr(eng_mod.Fit, k)) or isinstance(getattr(eng_mod.Fit, k), property))}
    own = {k for k in vars(eng_mod.Fit) if not k.startswith("_")}
    assert public - own == {"marginal"}
    assert {k for k in vars(eng_mod.FitViews) if not k.startswith("_")} == {"marginal"}
    assert eng_mod.Fit.__mro__[1:] == (eng_mod.FitViews, object)
