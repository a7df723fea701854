"""Joint posterior samples on the device (bq_gp_sample, engine.Fit.sample, gp.GP.sample) against
explicit CPU references.

The factor is held to its contract, not to another factor: L_c L_c^T must give back
Sigma_ref + jitter I, Sigma_ref from mpmath at 50 digits (n, M <= 65) or numpy.longdouble.  The
tolerance is measured, as in test_predict_grad.py: a float64 numpy route with the device's algebra
(Cholesky, triangular solve, Koo - V V^T, Cholesky with the device's jitter) gives
r = max |L L^T - (Sigma_ref + jitter I)| / T, T = max diag K(xo, xo) + max_i ||v_i||^2, and the
device gets 100 max(r, 4 eps) T.  Where numpy cannot factor its own Sigma at the jitter the device
used (a covariance singular in float64: which rung factors depends on rounding), r is that of its
Sigma alone.  The product is held to the gamma bound of an fp64 FMA chain on the mean and factor
the same call returned, the device normals to the numpy generator of test_gp_sample_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gp_sample_host import DEFAULT_LADDER, kernel_scale, normals
from test_predict_grad import _problem

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0
LD = np.longdouble


def _case(n, d, s, M, scale, on=0, dup=False):
    """The construction of test_predict_grad.py with the length scales times ``scale``; the first
    ``on`` query points are training points; dup: the last query point equals the first."""
    x, y, h, w, s = _problem(n, d, s, seed=n + 10 * d)
    w = w * scale
    xo = np.random.RandomState(1000 + n).uniform(-3.3, 3.3, size=(d, M))
    xo[:, :on] = x[:, :on]
    if dup:
        xo[:, -1] = xo[:, 0]
    return x, y, h, w, s, np.asfortranarray(xo)


def _mp_sigma(x, h, w, s, xo):
    """Sigma = Koo - Kox Kxx^-1 Kxo at 50 digits, rounded at the end."""
    import mpmath as mp
    mp.mp.dps = 50
    d, n = x.shape
    M = xo.shape[1]
    X = [[mp.mpf(float(x[k, i])) for k in range(d)] for i in range(n)]
    XO = [[mp.mpf(float(xo[k, j])) for k in range(d)] for j in range(M)]
    W = [mp.mpf(float(w[k])) for k in range(d)]
    c = mp.mpf(h) ** 2
    for k in range(d):
        c /= mp.sqrt(2 * mp.pi) * W[k]

    def kern(p, q):
        return c * mp.exp(-sum((p[k] - q[k]) ** 2 / (2 * W[k] ** 2) for k in range(d)))

    Kxx = mp.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):
            Kxx[i, j] = Kxx[j, i] = kern(X[i], X[j])
        Kxx[i, i] += mp.mpf(s) ** 2
    Kox = mp.matrix(M, n)
    for j in range(M):
        for i in range(n):
            Kox[j, i] = kern(XO[j], X[i])
    Sig = mp.matrix(M, M)
    for i in range(M):
        for j in range(i + 1):
            Sig[i, j] = Sig[j, i] = kern(XO[i], XO[j])
    Sig -= Kox * (Kxx ** -1) * Kox.T
    return np.array([[float(Sig[i, j]) for j in range(M)] for i in range(M)])


_LD_PI = LD(4) * np.arctan(LD(1))


def _ld_gram(a, b, h, w):
    c = LD(h) ** 2
    for wk in w:
        c /= np.sqrt(LD(2) * _LD_PI) * LD(wk)
    q = np.zeros((a.shape[1], b.shape[1]), dtype=LD)
    for k in range(a.shape[0]):
        t = a[k].astype(LD)[:, None] - b[k].astype(LD)[None, :]
        q += t * t / (LD(2) * LD(w[k]) ** 2)
    return c * np.exp(-q)


def _ld_sigma(x, h, w, s, xo):
    """The same in numpy.longdouble: an unblocked Cholesky of Kxx and a forward substitution."""
    n = x.shape[1]
    A = _ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD)
    Lf = np.zeros((n, n), dtype=LD)
    for j in range(n):
        Lf[j, j] = np.sqrt(A[j, j] - Lf[j, :j] @ Lf[j, :j])
        Lf[j + 1:, j] = (A[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    V = _ld_gram(xo, x, h, w)
    for j in range(n):  # V <- V L^-T, column by column
        V[:, j] = (V[:, j] - V[:, :j] @ Lf[j, :j]) / Lf[j, j]
    return (_ld_gram(xo, xo, h, w) - V @ V.T).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _reference(oracle, n, d, s, M, scale, on=0, dup=False):
    """(Sigma_ref, T, k0, Sigma_cpu): the reference, the size the bound is relative to, the prior
    variance as the library rounds it, and Sigma by the device's algebra in float64 numpy."""
    from scipy.linalg import solve_triangular
    x, y, h, w, s, xo = _case(n, d, s, M, scale, on, dup)
    sig = _mp_sigma(x, h, w, s, xo) if max(n, M) <= 65 else _ld_sigma(x, h, w, s, xo)
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    V = solve_triangular(Lc, np.ascontiguousarray(oracle.gram_cross(x, xo, h, w)), lower=True).T
    koo = np.asarray(oracle.gram(xo, h, w, 0.0))
    T = float(np.max(np.diag(koo)) + np.max(np.sum(V * V, axis=1)))
    cpu = koo - V @ V.T
    sig.setflags(write=False)  # shared among the tests of a case
    cpu.setflags(write=False)
    return sig, T, kernel_scale(h, w), cpu


def _factor_tol(ref, jitter, label):
    sig, T, k0, cpu = ref
    M = sig.shape[0]
    target = sig + jitter * np.eye(M)
    try:
        Lcpu = np.linalg.cholesky(cpu + jitter * np.eye(M))
        r = float(np.max(np.abs(Lcpu @ Lcpu.T - target))) / T
    except np.linalg.LinAlgError:  # (the module docstring says why this is not a failure)
        r = float(np.max(np.abs(cpu - sig))) / T
    print("%s: jitter/k0 %.3g, r %.3g" % (label, jitter / k0, r))
    return MARGIN * max(r, 4 * EPS) * T, target


def _check_factor(chol, ref, jitter, label):
    M = ref[0].shape[0]
    assert chol.shape == (M, M) and np.all(np.isfinite(chol))
    assert np.all(chol[np.triu_indices(M, 1)] == 0.0)
    tol, target = _factor_tol(ref, jitter, label)
    err = float(np.max(np.abs(chol @ chol.T - target)))
    print("%s: |L L^T - (Sigma_ref + jitter I)| / tol %.3g" % (label, err / tol))
    assert err <= tol, (label, err, tol)


# (n, d, s, M, w scale, leading query points on training points): M on both sides of the 16-row
# wave and the 64-row block, one, two, four and ten row blocks, lambda_min / k0 down to 1.5e-7
PD_CASES = [
    (40, 1, 0.3, 1, 1.0, 0), (40, 1, 0.3, 17, 0.1, 0), (70, 2, 0.05, 64, 0.5, 0),
    (130, 3, 1e-3, 65, 0.25, 16), (130, 3, 0.3, 130, 1.0, 0), (130, 3, 0.3, 200, 0.5, 0),
    (130, 3, 0.3, 600, 0.5, 0),
]
# Sigma singular in float64: (.., dup)
SINGULAR_CASES = [
    (40, 1, 0.3, 65, 1.0, 0, False), (40, 1, 0.0, 65, 0.25, 10, False),
    (130, 3, 0.3, 130, 1.0, 0, True),
]


@pytest.mark.parametrize("n,d,s,M,scale,on", PD_CASES)
def test_factor_of_a_definite_covariance_takes_no_jitter(engine, oracle, n, d, s, M, scale, on):
    ref = _reference(oracle, n, d, s, M, scale, on)
    lam = float(np.linalg.eigvalsh(ref[0])[0]) / ref[2]
    print("n=%d d=%d s=%g M=%d: lambda_min / k0 %.3g" % (n, d, s, M, lam))
    assert lam >= 1e-8
    x, y, h, w, s, xo = _case(n, d, s, M, scale, on)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        out, mean, jitter, chol = fit.sample(xo, S=2, seed=1, want_chol=True)
    finally:
        fit.close()
    assert jitter == 0.0 and out.shape == (M, 2) and mean.shape == (M,)
    _check_factor(chol, ref, jitter, "n=%d M=%d" % (n, M))


@pytest.mark.parametrize("n,d,s,M,scale,on,dup", SINGULAR_CASES)
def test_factor_of_a_singular_covariance_climbs_the_default_ladder(engine, oracle, n, d, s, M,
                                                                   scale, on, dup):
    ref = _reference(oracle, n, d, s, M, scale, on, dup)
    print("n=%d d=%d s=%g M=%d: lambda_min / k0 %.3g"
          % (n, d, s, M, float(np.linalg.eigvalsh(ref[0])[0]) / ref[2]))
    x, y, h, w, s, xo = _case(n, d, s, M, scale, on, dup)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        out, mean, jitter, chol = fit.sample(xo, S=2, seed=1, want_chol=True)  # status 0
    finally:
        fit.close()
    assert jitter in [ref[2] * t for t in DEFAULT_LADDER]
    assert np.all(np.isfinite(out))
    _check_factor(chol, ref, jitter, "n=%d M=%d" % (n, M))


def _raw(engine, fit, xo, M, S, z=None, seed=0, ladder=None, nl=0, out=None, mean=None, chol=None,
         jitter=None):
    dp = C.POINTER(C.c_double)

    def p(a):
        return None if a is None else a.ctypes.data_as(dp)

    return engine._lib.bq_gp_sample(engine._ctx, fit._handle(), p(xo), M, S, p(z), seed, p(ladder),
                                    nl, p(out), p(mean), p(chol), p(jitter))


def test_forced_ladder(engine, oracle):
    from bayesian_quadrature_amd import _lib
    case = (130, 3, 0.3, 130, 1.0)
    ref = _reference(oracle, *case)
    x, y, h, w, s, xo = _case(*case)
    k0, M = ref[2], 130
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        before = fit.predict(xo)[:2]
        out, mean, jitter, chol = fit.sample(xo, S=3, seed=2, ladder=(-0.5, 1e-3), want_chol=True)
        assert jitter == 1e-3 * k0
        _check_factor(chol, ref, jitter, "ladder (-0.5, 1e-3)")
        after = fit.predict(xo)[:2]
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        # every entry fails: BQ_ERR_NOT_PD and nothing written
        bufs = [np.full((M, 3), np.nan, order="F"), np.full(M, np.nan),
                np.full((M, M), np.nan, order="F"), np.full(1, np.nan)]
        st = _raw(engine, fit, xo, M, 3, ladder=np.array([-0.5]), nl=1, out=bufs[0], mean=bufs[1],
                  chol=bufs[2], jitter=bufs[3])
        assert st == _lib.BQ_ERR_NOT_PD == 1
        assert all(np.all(np.isnan(b)) for b in bufs)
        with pytest.raises(np.linalg.LinAlgError):
            fit.sample(xo, ladder=(-0.5,))
        after = fit.predict(xo)[:2]
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        fit.close()


def _product_bound(mean, chol, Z, extra=0.0):
    """(exact, bound): mean + L Z in long double and the gamma bound of an fp64 FMA chain of
    M + 1 terms in any order, (M + 4) eps (|mean_j| + sum_k |L_jk| |z_ks|), plus ``extra`` eps
    sum_k |L_jk| max(1, |z_ks|) for normals that are themselves a few ulp off."""
    M = mean.shape[0]
    Ll, Zl = chol.astype(LD), Z.astype(LD)
    exact = mean.astype(LD)[:, None] + Ll @ Zl
    bound = (M + 4) * EPS * (np.abs(mean).astype(LD)[:, None] + np.abs(Ll) @ np.abs(Zl))
    if extra:
        bound = bound + extra * EPS * (np.abs(Ll) @ np.maximum(1.0, np.abs(Zl)))
    return exact, bound


LINEAR_CASES = [(130, 3, 0.3, 130, 1.0), (40, 1, 0.3, 65, 1.0)]


@pytest.mark.parametrize("case", LINEAR_CASES)
def test_product_is_the_linear_map_of_the_returned_factor(engine, case):
    x, y, h, w, s, xo = _case(*case)
    assert np.any(y != 0)
    M = case[3]
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        pm = fit.predict(xo, want_mean=True, want_var=True)[0]
        for S in (1, 15, 16, 17, 70):
            Z = np.asfortranarray(np.random.RandomState(S).randn(M, S))
            out, mean, jitter, chol = fit.sample(xo, S=S, z=Z, want_chol=True)
            assert np.array_equal(mean, pm)
            exact, bound = _product_bound(mean, chol, Z)
            err = np.abs(out.astype(LD) - exact)
            print("M=%d S=%d: worst |out - (mean + L z)| / bound %.3g"
                  % (M, S, float(np.max(err / bound))))
            assert np.all(err <= bound)
        out, mean, _ = fit.sample(xo, S=17, z=np.zeros((M, 17)))
        assert np.array_equal(out, np.tile(mean[:, None], (1, 17)))
    finally:
        fit.close()


def test_sixteen_row_blocks(engine, oracle):
    """M = 1000, Mp = 1024: a leading dimension that is a large power of two, sixteen row blocks
    and two column chunks.  The factor's contract with whichever default jitter came back, and
    the product's bound on 70 columns."""
    case = (130, 3, 0.3, 1000, 0.5)
    ref = _reference(oracle, *case)
    x, y, h, w, s, xo = _case(*case)
    M, S = 1000, 70
    Z = np.asfortranarray(np.random.RandomState(5).randn(M, S))
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        out, mean, jitter, chol = fit.sample(xo, S=S, z=Z, want_chol=True)
        assert np.array_equal(mean, fit.predict(xo)[0])
    finally:
        fit.close()
    assert jitter in [ref[2] * t for t in DEFAULT_LADDER]
    _check_factor(chol, ref, jitter, "n=130 M=1000")
    exact, bound = _product_bound(mean, chol, Z)
    err = np.abs(out.astype(LD) - exact)
    print("M=%d S=%d: worst |out - (mean + L z)| / bound %.3g" % (M, S, float(np.max(err / bound))))
    assert np.all(err <= bound)


@pytest.mark.parametrize("case", LINEAR_CASES)
def test_device_normals_are_the_numpy_generator_s(engine, case):
    x, y, h, w, s, xo = _case(*case)
    M = case[3]
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        for S, seed in ((3, 7), (70, 7), (17, 12345678901234567)):
            out, mean, jitter, chol = fit.sample(xo, S=S, seed=seed, want_chol=True)
            Zr = normals(M, S, seed)
            exact, bound = _product_bound(mean, chol, Zr, extra=64.0)
            err = np.abs(out.astype(LD) - exact)
            print("M=%d S=%d seed=%d: worst error / bound %.3g"
                  % (M, S, seed, float(np.max(err / bound))))
            assert np.all(err <= bound)
            # the bound cannot hide a wrong normal: another seed's lie far outside it
            other = _product_bound(mean, chol, normals(M, S, seed + 1))[0]
            assert np.mean(np.abs(out.astype(LD) - other) > 1e6 * bound) > 0.9
        a, b = fit.sample(xo, S=5, seed=3), fit.sample(xo, S=5, seed=3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert not np.array_equal(a[0], fit.sample(xo, S=5, seed=4)[0])
        assert not np.array_equal(a[0], fit.sample(xo, S=5, seed=3 + 2 ** 32)[0])
    finally:
        fit.close()


def test_a_column_does_not_depend_on_the_number_of_columns(engine):
    x, y, h, w, s, xo = _case(40, 1, 0.3, 65, 1.0)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        a, b = fit.sample(xo, S=3, seed=7)[0], fit.sample(xo, S=70, seed=7)[0]
        assert a.shape == (65, 3) and b.shape == (65, 70)
        assert np.array_equal(a, b[:, :3])
        Z = np.asfortranarray(np.random.RandomState(0).randn(65, 70))
        a, b = fit.sample(xo, S=3, z=Z[:, :3])[0], fit.sample(xo, S=70, z=Z)[0]
        assert np.array_equal(a, b[:, :3])
    finally:
        fit.close()


def test_arguments(engine):
    from bayesian_quadrature_amd import _lib
    x, y, h, w, s, xo = _case(65, 2, 0.1, 65, 1.0)
    M = 65
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        before = fit.predict(xo)[:2]
        out = np.full((M, 2), np.nan, order="F")
        nan_ladder, ok_ladder = np.array([0.0, np.nan]), np.array([1e-6])
        big = np.zeros((2, 16385), order="F")
        bad = [
            dict(xo=xo, M=M, S=0, out=out),
            dict(xo=xo, M=M, S=4097, out=out),
            dict(xo=big, M=16385, S=1, out=out),
            dict(xo=xo, M=M, S=2, out=None),
            dict(xo=xo, M=M, S=2, out=out, ladder=nan_ladder, nl=2),
            dict(xo=xo, M=M, S=2, out=out, ladder=ok_ladder, nl=0),
            dict(xo=xo, M=-1, S=2, out=out),
        ]
        for kw in bad:
            assert _raw(engine, fit, **kw) == _lib.BQ_ERR_BAD_ARG == 2, kw
            after = fit.predict(xo)[:2]
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert np.all(np.isnan(out))
        assert _raw(engine, fit, xo=None, M=0, S=2, out=out) == _lib.BQ_OK == 0
        assert np.all(np.isnan(out))
        assert _raw(engine, fit, xo=xo, M=M, S=2, out=out) == 0 and np.all(np.isfinite(out))
        # the Python layer's own checks
        o, m, j = fit.sample(np.empty((2, 0)), S=3)
        assert o.shape == (0, 3) and m.shape == (0,)
        for call in (lambda: fit.sample(np.zeros((3, 4))), lambda: fit.sample(xo, S=0),
                     lambda: fit.sample(xo, S=2, z=np.zeros((M, 3))),
                     lambda: fit.sample(xo, seed=-1), lambda: fit.sample(xo, seed=2 ** 64),
                     lambda: fit.sample(xo, ladder=(0.0, np.inf))):
            with pytest.raises(ValueError):
                call()
        # new targets and no refit: the error predict gives
        fit.set_y(y + 1.0)
        errs = []
        for call in (lambda: fit.predict(xo), lambda: fit.sample(xo)):
            with pytest.raises(Exception) as ei:
                call()
            errs.append((type(ei.value), str(ei.value)))
        assert errs[0] == errs[1] and "refit" in errs[0][1]
        fit.refit(h, w, s)
        assert fit.sample(xo, S=2)[0].shape == (M, 2)
    finally:
        fit.close()


def test_gp_sample_on_the_device(engine):
    import bayesian_quadrature_amd as pkg
    rs = np.random.RandomState(3)
    x = np.sort(rs.uniform(-3, 3, size=40))
    y = np.sin(x) + 0.1 * rs.randn(40)
    g = pkg.GP(pkg.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    xo = np.linspace(-3, 3, 65)
    a, info = g.sample(xo, n=5, seed=11, return_info=True)
    assert a.shape == (5, 65) and np.all(np.isfinite(a))
    ref = g._fit.sample(xo, S=5, seed=11)
    assert np.array_equal(a, ref[0].T) and np.array_equal(info["mean"], ref[1])
    assert info["jitter"] == ref[2] and np.array_equal(info["mean"], g.mean_var(xo)[0])
    assert info["jitter"] in [kernel_scale(1.2, 0.8) * t for t in DEFAULT_LADDER]
    np.random.seed(77)
    b, c = g.sample(xo, n=2), g.sample(xo, n=2)
    assert b.shape == (2, 65) and not np.array_equal(b, c)
    np.random.seed(77)
    assert np.array_equal(g.sample(xo, n=2), b) and np.array_equal(g.sample(xo, n=2), c)
    z = rs.randn(4, 65)
    assert np.array_equal(g.sample(xo, n=4, z=z), g._fit.sample(xo, S=4, z=z.T)[0].T)
    g.set_param("h", 1.3)  # pending parameters are refitted first
    d = g.sample(xo, n=5, seed=11)
    fresh = pkg.GP(pkg.GaussianKernel(1.3, 0.8), x, y, s=0.2)
    assert np.array_equal(d, fresh.sample(xo, n=5, seed=11)) and not np.array_equal(d, a)
    assert g.sample([], n=3).shape == (3, 0)
