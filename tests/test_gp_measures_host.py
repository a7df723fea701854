"""CPU tests of the integrals and designs under the uniform measure on a box and under a mixture
of Gaussians: ld_measures.py's references held to independent derivations (mpmath quadrature), the
float64 yardsticks' error r recorded per family and dimension, the ``measures`` objects, and the
host plumbing -- engine.Fit.integral / integral_design as gp.GP.integral*, BQ.l_integral and
BQ.l_integral_design use them -- over a fit double that extends test_gp_zdesign_host.ZdFitDouble
with the yardsticks' kappa and kk.  test_gp_measures.py holds the device to the same references."""
import ctypes as C
import pickle

import mpmath
import numpy as np
import pytest

import ld_measures as lm
from engine_double import EngineDouble
from ld_closed_forms import EPS, LD, all_normal, ld_gram
from test_gp_pivchol_host import OPTIONS, _data
from test_gp_sample_host import kernel_scale
from test_gp_zdesign_host import ZdFitDouble, numpy_integral, numpy_zdesign, zvar_after


def _ms():
    from bayesian_quadrature_amd import measures
    return measures


class MeasureFitDouble(ZdFitDouble):
    """ZdFitDouble whose ``integral`` and ``integral_design`` take a measure object in place of
    mu, with engine.Fit's signatures: kappa and kk from ld_measures' float64 yardsticks."""

    def _kap(self, m):
        ms = _ms()
        if m.d != self.d:
            raise ValueError("dimension mismatch")
        if isinstance(m, ms.BoxMeasure):
            return (lambda p: lm.f64_box_kappa(self._pts(p), self.h, self.w, m.lo, m.hi),
                    float(lm.f64_box_kk(self.h, self.w, m.lo, m.hi)))
        for c in range(len(m)):
            try:
                np.linalg.cholesky(m.covs[c] + np.diag(self.w ** 2))
            except np.linalg.LinAlgError:
                raise ValueError("component %d's covariance plus diag(w^2) is not positive "
                                 "definite" % c)
        return (lambda p: lm.f64_mix_kappa(self._pts(p), self.h, self.w, m.weights, m.means,
                                           m.covs),
                float(lm.f64_mix_kk(self.h, self.w, m.weights, m.means, m.covs)))

    def integral(self, mu, cov=None, want_weights=False):
        if not isinstance(mu, _ms().Measure):
            return ZdFitDouble.integral(self, mu, cov, want_weights)
        if cov is not None:
            raise TypeError("a measure object comes without a cov")
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        kap, kk = self._kap(mu)
        self.calls.append(("integral", mu, None, want_weights, self.h))
        mean, var, wts = numpy_integral(kap(self.x), self.K(), self.y, kk)
        res = (float(mean), float(var))
        return res + (wts,) if want_weights else res

    def _u0m(self, xc, m):
        kap, kk = self._kap(m)
        wts = np.linalg.solve(np.asarray(self.K()), kap(self.x))
        Kcx = np.asarray(self.o.gram_cross(xc if self.d > 1 else xc[0], self.x, self.h, self.w))
        return kap(xc) - Kcx @ wts, kk - kap(self.x) @ wts, kk

    def integral_design(self, xc, q, mu, cov=None, nugget=0.0, tol=0.0, want_scores=False):
        if not isinstance(mu, _ms().Measure):
            return ZdFitDouble.integral_design(self, xc, q, mu, cov, nugget, tol, want_scores)
        if cov is not None:
            raise TypeError("a measure object comes without a cov")
        if self._L is None:
            raise ValueError("fit has new targets: refit required")
        xc = self._pts(xc)
        self.calls.append(("zdesign", xc.shape[1], q, nugget, tol, self.h, mu, None))
        u0, zvar0, kk = self._u0m(xc, mu)
        _, _, Sig = self.predict(xc if self.d > 1 else xc[0], want_cov=True)
        piv, gain, zvar0, ru, rc, s0, r = numpy_zdesign(
            np.asarray(Sig), u0, float(zvar0), kk, kernel_scale(self.h, self.w), q, nugget, tol)
        res = (piv[:r], gain[:r], float(zvar0), ru, rc)
        return res + (s0,) if want_scores else res


class MeasureEngineDouble(EngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return MeasureFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def pkg(oracle):
    import bayesian_quadrature_amd as pkg
    from bayesian_quadrature_amd import engine as eng_mod
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(MeasureEngineDouble(oracle), 0)
    yield pkg
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


# ---- the references and the yardsticks ----

@pytest.mark.parametrize("fam,d", [(f, d) for f in lm.BOX_FAMILIES for d in lm.box_dims(f)])
def test_box_reference_is_normal_and_the_yardstick_s_error(fam, d):
    """r per family and dimension at n = 40 (CPU, in eps: mild, edge, far, wide 1.1 .. 2.2; narrow
    1.3e3 .. 1.9e3 -- erf(b) + erf(-a) cancels where L / w = 1e-3, the contract's form; kk 0 .. 13)."""
    c = lm.box_case(fam, d, lm.N_HOST)
    assert c["ref"].shape == (lm.N_HOST,) and all_normal(c["ref"]) and all_normal(c["kk"])
    print("box %s d=%d: r %.1f eps, r_kk %.1f eps, smallest kappa %.3g"
          % (fam, d, c["r"] / EPS, c["r_kk"] / EPS, float(c["ref"].min())))
    assert np.isfinite(c["r"]) and np.isfinite(c["r_kk"])
    for n in lm.SIZES:   # the device's cases: normal too
        assert all_normal(lm.box_case(fam, d, n)["ref"])


@pytest.mark.parametrize("fam,d", [(f, d) for f in lm.MIX_FAMILIES for d in lm.DIMS])
def test_mixture_reference_is_normal_and_the_yardstick_s_error(fam, d):
    """r per family and dimension at n = 40 (CPU: 0.7 .. 5.8 eps; kk 0 .. 10 eps)."""
    c = lm.mix_case(fam, d, lm.N_HOST)
    assert c["ref"].shape == (lm.N_HOST,) and all_normal(c["ref"]) and all_normal(c["kk"])
    print("mix %s d=%d: r %.1f eps, r_kk %.1f eps" % (fam, d, c["r"] / EPS, c["r_kk"] / EPS))
    assert np.isfinite(c["r"]) and np.isfinite(c["r_kk"])
    for n in lm.SIZES:
        assert all_normal(lm.mix_case(fam, d, n)["ref"])
    if fam == "point":   # the point mass's share is pi_c times a gram_cross column
        w, pi, mu, cov = lm.mix_params(fam, d)
        only = lm.ld_mix_kappa(c["x"], c["h"], w, pi[1:2], mu[1:2], cov[1:2])
        col = LD(pi[1]) * ld_gram(c["x"], mu[1][:, None], c["h"], w)[:, 0]
        # (two long-double routes to one exponent q: each rounds it about d + 6 times -- the
        # differences, squares, scalings and sums -- and exp turns a relative rounding of q into
        # |q| times itself; |q| is at least |E| = |log(col / max col)|)
        E = np.abs(np.log(col / np.max(col)))
        assert float(np.max(np.abs(only - col) / col / (1 + E))) <= \
            2 * (d + 6) * float(np.finfo(LD).eps)


def _pieces(c, a, b, w, step=4, reach=12):
    """Break points of [a, b] for an integrand that lives within ``reach`` w of c (clamped into
    the interval: for a c outside, the tail's steep end is at the nearer edge)."""
    c = min(max(c, a), b)
    return sorted({a, b} | {min(max(c + j * step * w, a), b)
                            for j in range(-reach // step, reach // step + 1)})


@pytest.mark.parametrize("fam", lm.BOX_FAMILIES)
def test_box_reference_against_quadrature_in_one_dimension(fam):
    """kappa(t) = int k(t, x') dx' / L at three points, and kk = int int k / L^2 by a double
    mpmath.quad (Gauss-Legendre at 25 digits, in pieces of 4 w where the integrand lives; the
    inner integrand scaled by its largest value, since quad's error estimate is absolute)."""
    w, lo, hi, _ = lm.box_params(fam, 1)
    w, lo, hi = (mpmath.mpf(float(v[0])) for v in (w, lo, hi))
    h, L = mpmath.mpf(lm.H), hi - lo
    c = lm.box_case(fam, 1, lm.N_HOST)
    with mpmath.workdps(25):
        def k(a, b):
            return h * h * mpmath.npdf(a, b, w)

        def inner(t):
            peak = k(t, min(max(t, lo), hi))
            return peak * mpmath.quad(lambda xp: k(t, xp) / peak, _pieces(t, lo, hi, w),
                                      method="gauss-legendre")

        for i in (0, lm.N_HOST // 2, lm.N_HOST - 1):
            t = mpmath.mpf(float(c["x"][0, i]))
            assert abs(mpmath.mpf(str(c["ref"][i])) / (inner(t) / L) - 1) < 1e-17, (fam, i)
        outer = sorted(set(_pieces(lo, lo, hi, w)) | set(_pieces(hi, lo, hi, w)))
        kk = mpmath.quad(inner, outer, method="gauss-legendre") / (L * L)
        err = abs(mpmath.mpf(str(c["kk"])) / kk - 1)
        print("box %s: kk %s, closed form against quadrature %s" % (fam, mpmath.nstr(kk, 12),
                                                                     mpmath.nstr(err, 3)))
        assert err < 1e-17


def test_mixture_kk_against_quadrature_in_one_dimension():
    """ld_mix_kk's pair sum against kk = int int k m m by a double mpmath.quad (Gauss-Legendre at
    20 digits in pieces of 4 over [-12, 12]) for two broad components, 0.7 N(-0.8, 0.8^2) +
    0.4 N(1.1, 1.2^2) -- weights that do not sum to 1 --, h = 0.7, w = 0.9: all of the measure but
    e^-40 lies inside, and no piece holds a feature narrower than a quarter of it."""
    pi, mu, cov = np.array([0.7, 0.4]), np.array([[-0.8], [1.1]]), np.array([[[0.64]], [[1.44]]])
    w = np.array([0.9])
    got = lm.ld_mix_kk(lm.H, w, pi, mu, cov)
    cut = [mpmath.mpf(v) for v in range(-12, 13, 4)]
    with mpmath.workdps(20):
        h, wm = mpmath.mpf(lm.H), mpmath.mpf(float(w[0]))
        comp = [(mpmath.mpf(float(pi[j])), mpmath.mpf(float(mu[j, 0])),
                 mpmath.sqrt(mpmath.mpf(float(cov[j, 0, 0])))) for j in range(2)]

        def dens(x):
            return sum(p * mpmath.npdf(x, m, sd) for p, m, sd in comp)

        kk = mpmath.quad(lambda a: dens(a) * mpmath.quad(
            lambda b: h * h * mpmath.npdf(a, b, wm) * dens(b), cut, method="gauss-legendre"),
            cut, method="gauss-legendre")
        err = abs(mpmath.mpf(str(got)) / kk - 1)
        print("mixture: kk %s, pair sum against quadrature %s"
              % (mpmath.nstr(kk, 12), mpmath.nstr(err, 3)))
        assert err < 1e-16
    assert abs(LD(lm.f64_mix_kk(lm.H, w, pi, mu, cov)) - got) / got <= 16 * EPS


def test_box_integral_against_gauss_legendre(oracle):
    """mean = int m(x) dx / L and var = int int cov dx dx' / L^2 over [-4, 4] by a 200-node
    Gauss-Legendre rule on the posterior of a fit double (CPU: both to 4e-16)."""
    x, y = _data()
    fit = MeasureFitDouble(oracle, x, y, 1.2, 0.8, 0.2)
    box = _ms().BoxMeasure(-4.0, 4.0)
    mean, var, wts = fit.integral(box, want_weights=True)
    t, gw = np.polynomial.legendre.leggauss(200)
    xo, gw = 4.0 * t, gw / 2.0
    m, _, cov = fit.predict(xo, want_cov=True)
    em, ev = abs(mean - gw @ m), abs(var - gw @ np.asarray(cov) @ gw)
    print("box integral against Gauss-Legendre: mean %.3g, var %.3g" % (em, ev))
    assert em <= 1e-12 and ev <= 1e-12
    assert abs(wts @ y - mean) <= 1e-12 * np.abs(wts).dot(np.abs(y))


# ---- the measure objects ----

def test_measure_objects_are_checked_immutable_and_keyed():
    ms = _ms()
    b = ms.BoxMeasure([0.0, -1.0], [1.0, 2.0])
    assert b.d == 2 and isinstance(b.key, bytes) and b == ms.BoxMeasure((0, -1), (1, 2))
    assert ms.BoxMeasure(0.0, 1.0).d == 1
    with pytest.raises(AttributeError):
        b.lo = np.zeros(2)
    with pytest.raises(ValueError):
        b.lo[0] = 5.0
    for lo, hi in (([0.0], [0.0]), ([1.0], [0.0]), ([0.0, 0.0], [1.0]), ([np.nan], [1.0]),
                   ([0.0], [np.inf]), ([], [])):
        with pytest.raises(ValueError):
            ms.BoxMeasure(lo, hi)
    g = ms.GaussianMixture([0.5, 0.5], [-2.5, 2.5], [0.09, 0.09])
    assert g.d == 1 and len(g) == 2 and g.means.shape == (2, 1) and g.covs.shape == (2, 1, 1)
    g2 = ms.GaussianMixture([1.0, 2.0], [[0.0, 1.0], [1.0, 0.0]], np.zeros((2, 2, 2)))
    assert g2.d == 2 and g2.key != g.key
    with pytest.raises(AttributeError):
        g.weights = None
    with pytest.raises(ValueError):
        g.means[0, 0] = 1.0
    one = np.eye(2)[None]
    bad = [([], np.zeros((0, 2)), np.zeros((0, 2, 2))),                  # C < 1
           (np.ones(65), np.zeros((65, 1)), np.ones((65, 1, 1))),        # C > 64
           ([-0.1, 1.0], [0.0, 1.0], [1.0, 1.0]),                        # a negative weight
           ([0.0, 0.0], [0.0, 1.0], [1.0, 1.0]),                         # weights that sum to zero
           ([np.nan], [0.0], [1.0]), ([1.0], [np.inf], [1.0]), ([1.0], [0.0], [np.nan]),
           ([1.0], [[0.0, 0.0]], np.array([[[1.0, 0.5], [0.2, 1.0]]])),  # not symmetric
           ([1.0], [[0.0, 0.0]], np.ones((1, 3, 3))), ([1.0, 1.0], [[0.0, 0.0]], one)]
    for a in bad:
        with pytest.raises(ValueError):
            ms.GaussianMixture(*a)
    # the kind is part of the key: the same numbers are not the same measure
    assert ms.BoxMeasure([0.0], [1.0]).key != ms.GaussianMixture([1.0], [0.0], [1.0]).key
    for m in (b, g, g2):
        m2 = pickle.loads(pickle.dumps(m))
        assert m2 == m and m2.key == m.key and type(m2) is type(m)
    import bayesian_quadrature_amd as pkg
    assert pkg.BoxMeasure is ms.BoxMeasure and pkg.GaussianMixture is ms.GaussianMixture


# ---- the plumbing ----

def test_signatures_are_declared():
    from bayesian_quadrature_amd import _lib
    S = _lib.SIGNATURES
    box, mix = [_lib._dp] * 2, [C.c_int64] + [_lib._dp] * 3
    for name, tail in (("bq_gp_integral", 2), ("bq_gp_zdesign", 2), ("bq_int_K", 6)):
        res, args = S[name]
        head, rest = args[:tail], args[tail + 2:]   # (mu, cov) stand at `tail`
        extra = [_lib._dp] if name == "bq_int_K" else []   # kk
        for suffix, margs in (("_box", box), ("_mix", mix)):
            r2, a2 = S[name + suffix]
            assert r2 is res and a2 == head + margs + rest + extra, name + suffix
    from bayesian_quadrature_amd import engine
    import inspect
    assert list(inspect.signature(engine.Fit.integral).parameters) == \
        list(inspect.signature(MeasureFitDouble.integral).parameters)
    assert list(inspect.signature(engine.Fit.integral_design).parameters) == \
        list(inspect.signature(MeasureFitDouble.integral_design).parameters)


def _gp(pkg):
    x, y = _data()
    return pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2), x, y


def test_gp_integral_memoisation_per_measure_and_invalidation(pkg):
    g, x, y = _gp(pkg)
    box, box2 = pkg.BoxMeasure(-4.0, 4.0), pkg.BoxMeasure(0.0, 1.0)
    mix = pkg.GaussianMixture([0.5, 0.5], [-2.5, 2.5], [0.09, 0.09])
    a = g.integral(box)
    fit = g._fit
    n_calls = len(fit.calls)
    assert isinstance(a[0], float) and isinstance(a[1], float) and a[1] > 0
    assert g.integral(pkg.BoxMeasure([-4.0], [4.0])) == a and len(fit.calls) == n_calls
    wts = g.integral_weights(box)
    assert wts.shape == (40,) and len(fit.calls) == n_calls
    assert abs(wts @ y - a[0]) <= 1e-12 * np.abs(wts).dot(np.abs(y))
    assert fit.calls[-1][0] == "integral" and fit.calls[-1][1] is box and fit.calls[-1][3] is True
    # another measure, another kind and the Gaussian with the box's numbers: entries of their own
    b, c = g.integral(box2), g.integral(mix)
    e = g.integral(0.0, 1.0)
    assert len(fit.calls) == n_calls + 3 and len({a, b, c, e}) == 4
    assert g.integral(box) == a and g.integral(mix) == c and len(fit.calls) == n_calls + 3
    # the Gaussian call reaches the fit as (mu, cov), two positional arguments
    assert isinstance(fit.calls[-1][1], np.ndarray) and isinstance(fit.calls[-1][2], np.ndarray)
    # a parameter change refits and recomputes; new targets keep var and the weights
    g.set_param("h", 1.3)
    a2 = g.integral(box)
    assert a2 != a and fit.calls[-1][4] == 1.3
    w2 = g.integral_weights(box)
    g.y = 2.0 * y
    a3 = g.integral(box)
    assert abs(a3[0] - 2.0 * a2[0]) <= 1e-12 * abs(a2[0]) and abs(a3[1] - a2[1]) <= 1e-14
    assert np.allclose(g.integral_weights(box), w2, rtol=1e-12, atol=0)


def test_gp_integral_design_with_a_measure(pkg):
    g, x, y = _gp(pkg)
    mix = pkg.GaussianMixture([0.5, 0.5], [-2.5, 2.5], [0.09, 0.09])
    xo = np.linspace(-4.0, 4.0, 33)
    idx, info = g.integral_design(xo, 6, mix, return_info=True)
    call = g._fit.calls[-1]
    assert call[:5] == ("zdesign", 33, 6, 0.2 ** 2, 0.0) and call[6] is mix
    assert idx.shape == (6,) and idx.dtype == np.int64
    assert abs(info["zvar0"] - g.integral(mix)[1]) <= 1e-14
    sc = g.integral_scores(xo, mix)
    assert sc.shape == (33,) and int(np.argmax(sc)) == idx[0]
    idx2 = g.integral_design(xo, 6, mix, noisy=False)
    assert len(set(idx2.tolist())) == 6 and g._fit.calls[-1][3] == 0.0
    e, einfo = g.integral_design([], 3, mix, return_info=True)
    assert e.shape == (0,) and abs(einfo["zvar0"] - info["zvar0"]) <= 1e-14


def test_argument_errors(pkg):
    g, x, y = _gp(pkg)
    box = pkg.BoxMeasure(-4.0, 4.0)
    xo = np.array([0.1, 0.5, -2.0])
    for call in (lambda: g.integral(box, 1.0), lambda: g.integral_weights(box, [[1.0]]),
                 lambda: g.integral_design(xo, 2, box, 1.0),
                 lambda: g.integral_scores(xo, box, 1.0), lambda: g.integral(0.3)):
        with pytest.raises(TypeError):
            call()
    box2 = pkg.BoxMeasure([0.0, 0.0], [1.0, 1.0])
    for call in (lambda: g.integral(box2), lambda: g.integral_design(xo, 2, box2),
                 lambda: g.integral_design(xo, 4, box), lambda: g.integral_design(xo, 0, box),
                 lambda: g.integral_design(xo, 2, box, tol=-1.0)):
        with pytest.raises(ValueError):
            call()
    # a component whose covariance plus diag(w^2) is not positive definite: the integral's to say
    neg = pkg.GaussianMixture([1.0], [0.0], [-5.0])
    with pytest.raises(ValueError):
        g.integral(neg)
    # engine.Fit's own dispatch, without a device: the checks come before the library is touched
    from bayesian_quadrature_amd import engine

    class Bare(engine.Fit):
        def __init__(self):
            self.d, self.n, self._eng = 1, 3, None

        def __del__(self):
            pass

    f = Bare()
    with pytest.raises(TypeError):
        f.integral(box, [[1.0]])
    with pytest.raises(TypeError):
        f.integral_design(xo, 2, box, [[1.0]])
    with pytest.raises(TypeError):
        f.integral([0.3])
    with pytest.raises(ValueError):
        f.integral(box2)
    with pytest.raises(ValueError):
        f.integral_design(xo, 2, box2)
    for m in (box, pkg.GaussianMixture([1.0], [0.0], [1.0])):
        with pytest.raises(ValueError, match="single Gaussian"):
            f.sq_integral(m, None)
        with pytest.raises(ValueError, match="single Gaussian"):
            f.sq_integral_design(xo, 2, m, None)
        with pytest.raises(ValueError, match="single Gaussian"):
            g.sq_integral(m, None)
        with pytest.raises(ValueError, match="single Gaussian"):
            g.sq_integral_design(xo, 2, m, None)
    eng = engine.Engine.__new__(engine.Engine)
    with pytest.raises(TypeError):
        eng.int_K_box(xo, 1.0, [0.5], pkg.GaussianMixture([1.0], [0.0], [1.0]))
    with pytest.raises(TypeError):
        eng.int_K_mix(xo, 1.0, [0.5], box)
    with pytest.raises(ValueError):
        eng.int_K_box(xo, 1.0, [0.5], box2)


def test_gp_survives_pickling_after_a_measure_object(pkg):
    g, x, y = _gp(pkg)
    mix = pkg.GaussianMixture([0.5, 0.5], [-2.5, 2.5], [0.09, 0.0])
    a = g.integral(mix)
    g2 = pickle.loads(pickle.dumps(g))
    assert g2._memoized == {} and g2._fit is None   # only data and parameters travel
    assert g2.integral(pickle.loads(pickle.dumps(mix))) == a
    xo = np.linspace(-2, 2, 9)
    assert np.array_equal(g2.integral_design(xo, 3, mix), g.integral_design(xo, 3, mix))


def test_bq_l_integral_under_a_measure(pkg):
    import scipy.stats
    np.random.seed(8728)
    x = np.linspace(-5, 5, 9)
    bq = pkg.BQ(x, scipy.stats.norm.pdf(x, 0, 1), kernel=pkg.GaussianKernel, **OPTIONS)
    bq.init(params_tl=(15, 2, 0.1), params_l=(0.2, 1.3, 0))
    prior = bq.l_integral()
    assert prior == bq.l_integral(None) == bq.gp_l.integral(bq.options["x_mean"],
                                                            bq.options["x_cov"])
    box = pkg.BoxMeasure(-3.0, 3.0)
    got = bq.l_integral(box)
    assert got == bq.gp_l.integral(box) and got != prior
    # l is the standard normal density: its mean over [-3, 3] is (Phi(3) - Phi(-3)) / 6
    assert abs(got[0] - (scipy.stats.norm.cdf(3) - scipy.stats.norm.cdf(-3)) / 6) <= 5e-3
    x_c = np.linspace(-7, 7, 29)
    idx = bq.l_integral_design(x_c, 4, box)
    assert idx.shape == (4,) and bq.gp_l._fit.calls[-1][6] is box
    assert np.array_equal(idx, bq.gp_l.integral_design(x_c, 4, box))
    assert np.array_equal(bq.l_integral_design(x_c, 4), bq.l_integral_design(x_c, 4, None))
    with pytest.raises(TypeError):
        bq.l_integral((0.0, 1.0))
    with pytest.raises(ValueError):
        bq.l_integral(pkg.BoxMeasure([0.0, 0.0], [1.0, 1.0]))


# ---- the demonstrations ----

def test_a_measure_s_own_design_serves_it_best(pkg):
    """test_gp_zdesign_host.py's setting: 40 points, GaussianKernel(1.2, 0.8), s = 0.2, 33
    candidates on [-4, 4], six noisy picks.  Share of var Z left (CPU): the uniform measure on
    [-4, 4] under its own design 12.0 %, under the design for N(0, 1) 99.4 %; the mixture 0.5
    N(-2.5, 0.3^2) + 0.5 N(2.5, 0.3^2) under its own design 63.3 %, under the design for its
    moment-matched Gaussian 90.2 %.  Asserted: a measure's own design leaves no more of its own
    var Z than the other's."""
    g, x, y = _gp(pkg)
    xo = np.linspace(-4.0, 4.0, 33)
    nu = 0.2 ** 2
    box = pkg.BoxMeasure(-4.0, 4.0)
    mix = pkg.GaussianMixture([0.5, 0.5], [-2.5, 2.5], [0.3 ** 2, 0.3 ** 2])
    matched = (0.0, 2.5 ** 2 + 0.3 ** 2)
    Sig = np.asarray(g._device_fit().predict(xo, want_cov=True)[2])
    for name, own, other in (("box", box, (0.0, 1.0)), ("mixture", mix, matched)):
        mine = g.integral_design(xo, 6, own)
        theirs = g.integral_design(xo, 6, *other)
        u0, zvar0, kk = g._fit._u0m(xo[None, :], own)
        left = [zvar_after(Sig, u0, zvar0, P, nu) / zvar0 for P in (mine, theirs)]
        print("%s: its own design (at %s) leaves %.1f %% of var Z, the design for N(%g, %g) (at "
              "%s) %.1f %%" % (name, xo[mine], 100 * left[0], other[0], other[1], xo[theirs],
                               100 * left[1]))
        assert abs(zvar0 - g.integral(own)[1]) <= 1e-14
        assert left[0] <= left[1]
