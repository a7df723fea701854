"""The integral of a resident fit and the designs that lower its variance on the device
(bq_gp_integral, bq_gp_zdesign; engine.Fit.integral, engine.Fit.integral_design) against explicit
CPU references.

Points are test_gp_sample.py's ``_case(n, d, s, A, scale)``, whose ``_reference`` gives Sigma_ref
(numpy.longdouble) over the candidates; the measure is mu_k = 0.25 (-1)^k, Sigma = 1.5^2 (0.7 I +
0.3 1 1^T), correlated and off-centre.  kappa, kk, Kxx^-1 kappa_X and u0 come from the closed
forms in long double (``_ld_kappa``, test_gp_pivchol._ld_solve_spd).

The device is held to the recurrence of include/bqhip.h in long double along the device's own
pivots (``_along``): gain, zvar0, resid_u, resid_c and score0.  Each device pivot is greedy within
the tolerance, and zvar0 - sum gain is the long-double variance of Z after the steps.  The pivots
equal those of the free long-double recurrence after the test has asserted, on the reference alone,
that every step's best score leads the second by at least LEAD = 1000 tolerances, that every gain is
positive and that the smallest eligible dc + nugget stays above 1.5e-3 k0.

The tolerances are measured, as in test_gp_ivr.py: the float64 restatement
(test_gp_zdesign_host.numpy_zdesign) runs on the device's algebra -- the oracle's Gram, Cholesky,
triangular solve, int_K and K - V V^T -- along the device's pivots, and its largest error against
the long-double recurrence gives r relative to the size of the terms: T = max diag K +
max_i ||v_i||^2 for the variances, kk + |b|^2 for var Z, U = max kappa + max_i ||v_i|| |b| for u,
and U^2 over the smallest eligible dc + nugget for scores and gains.  The device gets
100 max(r, 4 eps) times that scale."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gp_pivchol import _ld_solve_spd
from test_gp_sample import _LD_PI, _case, _ld_gram, _ld_sigma, _reference
from test_gp_sample_host import kernel_scale
from test_gp_zdesign_host import numpy_zdesign

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0
LD = np.longdouble

LEAD = 1000.0

# (n, d, s, A, w scale, q, noisy, seed): one row block; four row blocks with and without a nugget;
# six row blocks and npad + q past 256 (n = 200: npad = 256); d = 1; a single candidate.  seed
# None: _case's candidates.  Every case keeps its q and leads by LEAD tolerances at every step.
# One case draws its candidates from a seed of its own, RandomState(seed).uniform(-3.3, 3.3): with
# _case's, one candidate of (130, 2, 0.05, 70) lies so close to an observation that its variance
# without a nugget is 1.35e-3 k0 (about s^2) from step 0 on, below the 1.5e-3 k0 that the
# comparison asks of the smallest eligible dc + nugget.  Seed 14 is the one of 1 .. 14 with the
# widest margins on the reference: a lead of 1.8e4 tolerances, dc of at least 2.3e-3 k0.
CASES = [
    (65, 3, 0.1, 64, 1.0, 16, True, None),
    (130, 3, 0.1, 200, 1.0, 24, True, None),
    (130, 3, 0.1, 200, 1.0, 24, False, None),
    (130, 2, 0.05, 70, 0.5, 32, True, None),
    (130, 2, 0.05, 70, 0.5, 32, False, 14),
    (200, 3, 0.1, 330, 1.0, 40, True, None),
    (65, 1, 0.1, 64, 0.25, 12, True, None),
    (70, 2, 0.05, 63, 0.5, 9, False, None),
    (70, 2, 0.05, 1, 0.5, 1, True, None),
]


def _points(n, d, s, A, scale, seed=None):
    x, y, h, w, s, xc = _case(n, d, s, A, scale)
    if seed is not None:
        xc = np.asfortranarray(np.random.RandomState(seed).uniform(-3.3, 3.3, size=(d, A)))
    return x, y, h, w, s, xc


def _sigma(oracle, n, d, s, A, scale, seed):
    """test_gp_sample._reference's (Sigma_ref, T, k0, Sigma_cpu), also for candidates of a seed
    of their own."""
    if seed is None:
        return _reference(oracle, n, d, s, A, scale)
    from scipy.linalg import solve_triangular
    x, y, h, w, s, xc = _points(n, d, s, A, scale, seed)
    sig = _ld_sigma(x, h, w, s, xc)
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    V = solve_triangular(Lc, np.ascontiguousarray(oracle.gram_cross(x, xc, h, w)), lower=True).T
    koo = np.asarray(oracle.gram(xc, h, w, 0.0))
    T = float(np.max(np.diag(koo)) + np.max(np.sum(V * V, axis=1)))
    return sig, T, kernel_scale(h, w), koo - V @ V.T


def _measure(d):
    mu = np.array([0.25 * (-1) ** k for k in range(d)])
    cov = 1.5 ** 2 * (0.7 * np.eye(d) + 0.3 * np.ones((d, d)))
    return mu, np.asfortranarray(cov)


def _nu(s, noisy):
    return s * s if noisy else 0.0


def _ld_chol(Am):
    n = Am.shape[0]
    Lf = np.zeros((n, n), dtype=LD)
    for j in range(n):
        Lf[j, j] = np.sqrt(Am[j, j] - Lf[j, :j] @ Lf[j, :j])
        Lf[j + 1:, j] = (Am[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return Lf


def _ld_kappa(pts, h, w, mu, cov, factor=1):
    """h^2 N(pts_i | mu, diag(w^2) + factor cov) in long double; pts None: h^2 N(0 | 0, .)."""
    d = len(w)
    Cm = LD(factor) * cov.astype(LD) + np.diag(np.asarray(w, dtype=LD) ** 2)
    Lf = _ld_chol(Cm)
    logc = -LD(d) / 2 * np.log(LD(2) * _LD_PI) - np.sum(np.log(np.diag(Lf)))
    if pts is None:
        return LD(h) ** 2 * np.exp(logc)
    z = pts.astype(LD) - mu.astype(LD)[:, None]
    for j in range(d):
        z[j] = (z[j] - Lf[j, :j] @ z[:j]) / Lf[j, j]
    return LD(h) ** 2 * np.exp(logc - np.sum(z * z, axis=0) / 2)


@functools.lru_cache(maxsize=None)
def _pieces(oracle, n, d, s, A, scale, seed=None):
    """What the tests of a case share: {"ld": the long-double kappa_X, kk, weights, u0, zvar0,
    mean; "f64": the same by the device's algebra in float64; the scales T, U, Zs; k0}."""
    from scipy.linalg import solve_triangular
    x, y, h, w, s, xc = _points(n, d, s, A, scale, seed)
    mu, cov = _measure(d)
    sig, T, k0, cpu = _sigma(oracle, n, d, s, A, scale, seed)
    Am = _ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD)
    kx, kc = _ld_kappa(x, h, w, mu, cov), _ld_kappa(xc, h, w, mu, cov)
    kk = _ld_kappa(None, h, w, mu, cov, 2)
    om = _ld_solve_spd(Am, kx)
    ld = dict(kk=kk, weights=om, u0=kc - _ld_gram(xc, x, h, w) @ om, zvar0=kk - kx @ om,
              mean=y.astype(LD) @ om)
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    V = solve_triangular(Lc, np.ascontiguousarray(oracle.gram_cross(x, xc, h, w)), lower=True).T
    b = solve_triangular(Lc, oracle.int_K(x, h, w, mu, cov), lower=True)
    z = solve_triangular(Lc, y, lower=True)
    kc64 = oracle.int_K(xc, h, w, mu, cov)
    kk64 = oracle.int_int_K(d, h, w, mu, cov)
    f64 = dict(kk=kk64, weights=solve_triangular(Lc.T, b, lower=False), u0=kc64 - V @ b,
               zvar0=kk64 - b @ b, mean=b @ z)
    vn = np.sqrt(np.max(np.sum(V * V, axis=1)))
    out = dict(ld=ld, f64=f64, T=T, k0=k0, sig=sig, cpu=cpu,
               U=float(np.max(kc64) + vn * np.linalg.norm(b)), Zs=float(kk64 + b @ b),
               Ms=float(np.linalg.norm(b) * np.linalg.norm(z)))
    for v in list(ld.values()) + list(f64.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _along(sig, u0, zvar0, piv, nu):
    """The recurrence along the pivots ``piv`` in long double: {"scores": every step's score
    vector, -inf where not eligible; "gain"; "zvar": var Z before every step and after the last;
    "den2": every step's smallest eligible dc + nu; "u"; "dc"}."""
    S = sig.astype(LD)
    u, dc = u0.astype(LD).copy(), np.diag(S).copy()
    A, q = S.shape[0], len(piv)
    Cf = np.zeros((A, q), dtype=LD)
    taken = np.zeros(A, dtype=bool)
    out = {"scores": [], "gain": [], "zvar": [LD(zvar0)], "den2": []}
    for t, p in enumerate(piv):
        den2 = dc + LD(nu)
        ok = (den2 > 0) & ~taken if nu == 0 else den2 > 0
        sc = np.full(A, -np.inf, dtype=LD)
        sc[ok] = u[ok] * u[ok] / den2[ok]
        out["scores"].append(sc)
        out["gain"].append(sc[p])
        out["den2"].append(den2[ok].min())
        den = np.sqrt(den2[p])
        c = (S[:, p] - Cf[:, :t] @ Cf[p, :t]) / den
        coef = u[p] / den
        if nu == 0:
            c[taken] = 0
            c[p] = den
            taken[p] = True
        u = u - c * coef
        dc = dc - c * c
        if nu == 0:
            dc[taken] = 0
            u[taken] = 0
        Cf[:, t] = c
        out["zvar"].append(out["zvar"][-1] - sc[p])
    out["gain"] = np.array(out["gain"], dtype=LD)
    out["u"], out["dc"] = u, dc
    return out


def _errors(dev, ld):
    """(error of gain and score0, of zvar0, of resid_u, of resid_c) of a result (piv, gain, zvar0,
    resid_u, resid_c, score0) against _along's."""
    piv, gain, zvar0, ru, rc, s0 = dev
    s0_ld = np.where(np.isfinite(ld["scores"][0]), ld["scores"][0], 0) if len(piv) else s0
    eg = max(float(np.max(np.abs(gain - ld["gain"]))) if len(piv) else 0.0,
             float(np.max(np.abs(s0 - s0_ld))))
    return (eg, float(abs(zvar0 - ld["zvar"][0])), float(np.max(np.abs(ru - ld["u"]))),
            float(np.max(np.abs(rc - ld["dc"]))))


def _tolerance(pc, piv, nu, ld, label):
    """(tol for gains and scores, for var Z, for u, for variances): 100 max(r, 4 eps) times the
    scales of the module docstring, r from the float64 restatement on the device's algebra along
    the device's pivots."""
    f64, T, U, Zs = pc["f64"], pc["T"], pc["U"], pc["Zs"]
    G = U * U / float(min(ld["den2"])) if len(piv) else U * U / pc["k0"]
    out = numpy_zdesign(np.array(pc["cpu"]), f64["u0"], f64["zvar0"], f64["kk"], pc["k0"], len(piv),
                        nu, 0.0, pivots=piv)
    r = max(float(np.max(np.abs(pc["cpu"] - pc["sig"]))) / T,
            float(np.max(np.abs(f64["u0"] - pc["ld"]["u0"]))) / U,
            float(abs(f64["zvar0"] - pc["ld"]["zvar0"])) / Zs)
    if out[6] == len(piv):
        eg, ez, eu, ev = _errors((piv,) + out[1:6], ld)
        r = max(r, eg / G, ez / Zs, eu / U, ev / T)
    print("%s: r %.3g" % (label, r))
    m = MARGIN * max(r, 4 * EPS)
    return m * G, m * Zs, m * U, m * T


@functools.lru_cache(maxsize=None)
def _device(engine, n, d, s, A, scale, q, noisy, seed=None):
    x, y, h, w, s, xc = _points(n, d, s, A, scale, seed)
    mu, cov = _measure(d)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        out = fit.integral_design(xc, q, mu, cov, nugget=_nu(s, noisy), want_scores=True)
    finally:
        fit.close()
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("n,d,s,A,scale,q,noisy,seed", CASES)
def test_design_holds_its_contract(engine, oracle, n, d, s, A, scale, q, noisy, seed):
    pc = _pieces(oracle, n, d, s, A, scale, seed)
    nu = _nu(s, noisy)
    dev = _device(engine, n, d, s, A, scale, q, noisy, seed)
    piv, gain, zvar0, ru, rc, s0 = dev
    label = "n=%d d=%d A=%d q=%d nu=%g" % (n, d, A, q, nu)
    assert piv.shape == (q,) and piv.dtype == np.int64 and gain.shape == (q,)  # full rank
    assert ru.shape == (A,) and rc.shape == (A,) and s0.shape == (A,) and isinstance(zvar0, float)
    assert np.all((piv >= 0) & (piv < A)) and np.all(gain > 0)
    assert np.all(np.isfinite(ru)) and np.all(np.isfinite(rc)) and np.all(np.isfinite(s0))
    assert s0[piv[0]] == gain[0] == s0.max() and piv[0] == int(np.argmax(s0))
    ld = _along(pc["sig"], pc["ld"]["u0"], pc["ld"]["zvar0"], piv, nu)
    tg, tz, tu, tv = _tolerance(pc, piv, nu, ld, label)
    eg, ez, eu, ev = _errors(dev, ld)
    short = max(float(np.max(sc) - sc[p]) for sc, p in zip(ld["scores"], piv))
    # every term of zvar0 - sum gain is within its tolerance of its exact value
    tele = abs(float(zvar0 - float(np.sum(gain)) - ld["zvar"][-1]))
    print("%s: gain error / tol %.3g, var Z error / tol %.3g, u error / tol %.3g, variance error "
          "/ tol %.3g, greedy shortfall / tol %.3g, telescoping / tol %.3g, smallest gain / kk %.3g"
          % (label, eg / tg, ez / tz, eu / tu, ev / tv, short / tg, tele / (tz + q * tg),
             float(np.min(gain)) / pc["f64"]["kk"]))
    assert eg <= tg and ez <= tz and eu <= tu and ev <= tv and short <= tg
    assert tele <= tz + q * tg
    if nu == 0.0:
        assert len(set(piv.tolist())) == q and np.all(rc[piv] == 0.0) and np.all(ru[piv] == 0.0)
    else:
        assert np.all(rc > 0)


@pytest.mark.parametrize("n,d,s,A,scale,q,noisy,seed", CASES)
def test_pivots_are_the_reference_s(engine, oracle, n, d, s, A, scale, q, noisy, seed):
    pc = _pieces(oracle, n, d, s, A, scale, seed)
    nu = _nu(s, noisy)
    want, wgain, _, _, _, _, rank = numpy_zdesign(
        pc["sig"].astype(LD), pc["ld"]["u0"], pc["ld"]["zvar0"], pc["ld"]["kk"], LD(pc["k0"]), q,
        nu, 0.0)
    assert rank == q and np.all(wgain > 0)
    # the conditions that make the comparison fair, on the reference alone
    ld = _along(pc["sig"], pc["ld"]["u0"], pc["ld"]["zvar0"], want, nu)
    leads = []
    for sc, p in zip(ld["scores"], want):
        rest = np.delete(sc, p)
        rest = rest[np.isfinite(rest)]
        leads.append(float(sc[p] - np.max(rest)) if rest.size else np.inf)
    tg = _tolerance(pc, want, nu, ld, "n=%d d=%d A=%d q=%d nu=%g" % (n, d, A, q, nu))[0]
    den2 = float(min(ld["den2"]))
    kk = float(pc["ld"]["kk"])
    print("smallest lead %.3g kk = %.3g tol, smallest dc + nu %.3g k0, smallest gain %.3g kk"
          % (min(leads) / kk, min(leads) / tg, den2 / pc["k0"], float(np.min(wgain)) / kk))
    assert min(leads) >= LEAD * tg
    assert den2 >= 1.5e-3 * pc["k0"]
    piv, gain = _device(engine, n, d, s, A, scale, q, noisy, seed)[:2]
    assert np.array_equal(piv, want)
    assert float(np.max(np.abs(gain - wgain.astype(np.float64)))) <= tg


def test_prefix_property_same_bits_and_predict_s_variance(engine):
    n, d, s, A, scale, q = 130, 3, 0.1, 200, 1.0, 24
    x, y, h, w, s, xc = _case(n, d, s, A, scale)
    mu, cov = _measure(d)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        for nu in (0.0, s * s):
            full = fit.integral_design(xc, q, mu, cov, nugget=nu, want_scores=True)
            again = fit.integral_design(xc, q, mu, cov, nugget=nu, want_scores=True)
            assert all(np.array_equal(a, b) for a, b in zip(full, again))
            for j in (1, q // 2, 17, q):
                part = fit.integral_design(xc, j, mu, cov, nugget=nu, want_scores=True)
                assert np.array_equal(part[0], full[0][:j])
                assert np.array_equal(part[1], full[1][:j])
                assert part[2] == full[2] and np.array_equal(part[5], full[5])
            bare = fit.integral_design(xc, q, mu, cov, nugget=nu)
            assert len(bare) == 5 and all(np.array_equal(a, b) for a, b in zip(bare, full))
        # the sweep under it is bq_gp_predict's: a stop level above every gain leaves dc^0, its
        # variance bits, and zvar0 is bq_gp_integral's var
        var = fit.predict(xc)[1]
        p0, g0, zvar0, ru, rc = fit.integral_design(xc, 1, mu, cov, tol=1e6)
        assert p0.shape == (0,) and g0.shape == (0,) and np.array_equal(rc, var)
        assert zvar0 == fit.integral(mu, cov)[1]
        # stop rule: a level just above the third gain (the first of the run below both before it)
        g = full[1]
        j = next(i for i in range(1, q) if g[i] < g[:i].min())
        kk = float(_ld_kappa(None, h, w, mu, cov, 2))
        lvl = float(g[j]) * (1 + 1e-9) / kk
        piv, gain, _, _, _ = fit.integral_design(xc, q, mu, cov, nugget=s * s, tol=lvl)
        assert piv.shape == (j,) and np.array_equal(piv, full[0][:j])
        assert np.array_equal(gain, full[1][:j])
    finally:
        fit.close()


def test_stop_rule_after_three_steps(engine):
    """tol just above the third gain: rank 3 and piv[3:] = -1 through the C entry point."""
    n, d, s, A, scale, q = 65, 3, 0.1, 64, 1.0, 8
    x, y, h, w, s, xc = _case(n, d, s, A, scale)
    mu, cov = _measure(d)
    kk = float(_ld_kappa(None, h, w, mu, cov, 2))
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        full = fit.integral_design(xc, q, mu, cov, nugget=s * s)
        g = full[1]
        assert g[3] < g[:3].min()  # (else the level below would end the run earlier)
        o = _outs(q, A)
        st = _raw(engine, fit, mu, cov, xc, A, q, s * s, float(g[3]) * (1 + 1e-9) / kk, o)
        assert st == 0 and o["rank"][0] == 3 and np.all(o["piv"][3:] == -1)
        assert np.array_equal(o["piv"][:3], full[0][:3]) and np.all(o["gain"][3:] == 0.0)
        assert np.array_equal(o["gain"][:3], g[:3])
    finally:
        fit.close()


def test_noisy_gains_are_the_variance_after_append(engine, oracle):
    """With nugget = s^2, zvar0 - sum gain[:t] is the var bq_gp_integral returns after append of
    the first t picks with arbitrary targets; both are held to the long-double recurrence."""
    n, d, s, A, scale, q, t = 130, 3, 0.1, 200, 1.0, 24, 10
    pc = _pieces(oracle, n, d, s, A, scale)
    x, y, h, w, s, xc = _case(n, d, s, A, scale)
    mu, cov = _measure(d)
    piv, gain, zvar0 = _device(engine, n, d, s, A, scale, q, True)[:3]
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        fit.append(np.asfortranarray(xc[:, piv[:t]]), np.random.RandomState(5).randn(t))
        mean, var, wts = fit.integral(mu, cov, want_weights=True)
    finally:
        fit.close()
    ld = _along(pc["sig"], pc["ld"]["u0"], pc["ld"]["zvar0"], piv, s * s)
    tg, tz, _, _ = _tolerance(pc, piv, s * s, ld, "append")
    e1 = abs(float(zvar0 - np.sum(gain[:t]) - ld["zvar"][t]))
    e2 = abs(float(var - ld["zvar"][t]))
    print("after %d picks: telescoped error / tol %.3g, appended error / tol %.3g"
          % (t, e1 / (tz + t * tg), e2 / tz))
    assert e1 <= tz + t * tg and e2 <= tz
    assert abs(var - (zvar0 - np.sum(gain[:t]))) <= 2 * tz + t * tg
    assert wts.shape == (n + t,) and np.isfinite(mean)


@pytest.mark.parametrize("n,d,s,A,scale", [(65, 3, 0.1, 64, 1.0), (130, 2, 0.05, 70, 0.5),
                                            (200, 3, 0.1, 330, 1.0), (65, 1, 0.1, 64, 0.25)])
def test_integral_against_long_double(engine, oracle, n, d, s, A, scale):
    pc = _pieces(oracle, n, d, s, A, scale)
    x, y, h, w, s, xc = _case(n, d, s, A, scale)
    mu, cov = _measure(d)
    ld, f64 = pc["ld"], pc["f64"]
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        mean, var, wts = fit.integral(mu, cov, want_weights=True)
        assert fit.integral(mu, cov) == (mean, var)  # the state is there: the same bits
        m_only = fit.integral(mu, cov)[0]
        zm = engine.Z_mean(fit, mu, cov)
    finally:
        fit.close()
    Ws = float(np.max(np.abs(f64["weights"])))
    Ys = float(np.abs(f64["weights"]) @ np.abs(y))
    rm = abs(float(f64["mean"] - ld["mean"])) / pc["Ms"]
    rz = abs(float(f64["zvar0"] - ld["zvar0"])) / pc["Zs"]
    rw = float(np.max(np.abs(f64["weights"] - ld["weights"]))) / Ws
    tm, tz, tw = (MARGIN * max(r, 4 * EPS) * sc for r, sc in ((rm, pc["Ms"]), (rz, pc["Zs"]), (rw, Ws)))
    em, ez = abs(float(mean - ld["mean"])), abs(float(var - ld["zvar0"]))
    ew = float(np.max(np.abs(wts - ld["weights"])))
    print("n=%d d=%d: r mean %.3g var %.3g weights %.3g; error / tol mean %.3g var %.3g weights "
          "%.3g" % (n, d, rm, rz, rw, em / tm, ez / tz, ew / tw))
    assert em <= tm and ez <= tz and ew <= tw and m_only == mean
    # Z_mean is the same number by another route (alpha . kappa_X): its error is the weights'
    assert abs(zm - mean) <= tm + tw * float(np.sum(np.abs(y)))
    assert abs(float(wts @ y) - mean) <= tm + n * EPS * Ys + tw * float(np.sum(np.abs(y)))


def _twins(engine, n=130, d=3, s=0.1, A=8, scale=1.0):
    x, y, h, w, s, xc = _case(n, d, s, A, scale)
    return (x, y, h, w, s, xc) + _measure(d)


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_derived_state_follows_the_events(engine):
    """The KMEAN row of the derived-state table, with twins as in test_gp_fit_state.py: a warm fit
    that has computed the integral before the event against a cold one that computes it after."""
    x, y, h, w, s, xc, mu, cov = _twins(engine)
    mu2, cov2 = mu + 0.5, np.asfortranarray(cov * 0.5)
    y2 = np.cos(y) + 0.3
    rs = np.random.RandomState(11)
    xn, yn = np.asfortranarray(rs.uniform(-3, 3, size=(x.shape[0], 5))), rs.randn(5)

    def events():
        yield "set_y", lambda f: (f.set_y(y2), f.refit(h, w, s))
        yield "refit", lambda f: f.refit(1.1 * h, 0.9 * w, s)
        yield "append", lambda f: f.append(xn, yn)
        yield "remove", lambda f: f.remove(np.array([3, 64, 100]))

    for name, ev in events():
        warm, cold = engine.gp_fit(x, y, h, w, s), engine.gp_fit(x, y, h, w, s)
        try:
            before = warm.integral(mu, cov, want_weights=True)
            ev(warm), ev(cold)
            a = warm.integral(mu, cov, want_weights=True)
            b = cold.integral(mu, cov, want_weights=True)
            assert _same(a, b), name
            if name == "set_y":  # b does not depend on the targets
                assert a[1] == before[1] and np.array_equal(a[2], before[2]) and a[0] != before[0]
                fresh = engine.gp_fit(x, y2, h, w, s)
                try:
                    assert _same(fresh.integral(mu, cov, want_weights=True), a)
                finally:
                    fresh.close()
            else:
                assert a[1] != before[1]
            # the design computes the state on its way where it is not there
            da = warm.integral_design(xc, 4, mu2, cov2)
            db = cold.integral_design(xc, 4, mu2, cov2)
            assert all(np.array_equal(u, v) for u, v in zip(da, db)), name
            assert da[2] == warm.integral(mu2, cov2)[1]
        finally:
            warm.close(), cold.close()
    # a second key recomputes; going back gives the first bits
    f = engine.gp_fit(x, y, h, w, s)
    try:
        a = f.integral(mu, cov, want_weights=True)
        b = f.integral(mu2, cov2, want_weights=True)
        assert not _same(a, b)
        assert _same(f.integral(mu, cov, want_weights=True), a)
        assert _same(f.integral(mu2, cov2, want_weights=True), b)
    finally:
        f.close()


def _outs(q, A):
    return dict(piv=np.full(q, 7, dtype=np.int64), gain=np.full(q, 7.0), zvar0=np.full(1, 7.0),
                ru=np.full(A, 7.0), rc=np.full(A, 7.0), s0=np.full(A, 7.0),
                rank=np.full(1, 7, dtype=np.int64))


def _raw(engine, fit, mu, cov, xc, A, q, nugget, tol, o):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def p(a, t=dp):
        return None if a is None else a.ctypes.data_as(t)

    return engine._lib.bq_gp_zdesign(engine._ctx, fit._handle(), p(mu), p(cov), p(xc), A, q, nugget,
                                     tol, p(o["piv"], ip), p(o["gain"]), p(o["zvar0"]), p(o["ru"]),
                                     p(o["rc"]), p(o["s0"]), p(o["rank"], ip))


def _raw_integral(engine, fit, mu, cov, mean, var, wts):
    dp = C.POINTER(C.c_double)

    def p(a):
        return None if a is None else a.ctypes.data_as(dp)

    return engine._lib.bq_gp_integral(engine._ctx, fit._handle(), p(mu), p(cov), p(mean), p(var),
                                      p(wts))


def test_argument_errors_write_nothing(engine):
    x, y, h, w, s, xc = _case(40, 2, 0.3, 10, 1.0)
    A, n = 10, 40
    mu, cov = _measure(2)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        def call(o, **kw):
            a = dict(mu=mu, cov=cov, xc=xc, A=A, q=4, nugget=0.0, tol=0.0)
            a.update(kw)
            return _raw(engine, fit, a["mu"], a["cov"], a["xc"], a["A"], a["q"], a["nugget"],
                        a["tol"], o)

        def bad_mu(v):
            b = mu.copy()
            b[1] = v
            return b

        def bad_cov(v):
            b = cov.copy(order="F")
            b[0, 1] = b[1, 0] = v
            return b

        not_pd = np.asfortranarray(-10.0 * np.eye(2))
        bad = [dict(A=-1), dict(q=0), dict(q=-3), dict(q=A + 1), dict(nugget=-1e-3),
               dict(nugget=np.nan), dict(nugget=np.inf), dict(tol=-1e-3), dict(tol=np.nan),
               dict(tol=np.inf), dict(mu=None), dict(cov=None), dict(xc=None),
               dict(mu=bad_mu(np.nan)), dict(mu=bad_mu(np.inf)), dict(cov=bad_cov(np.nan)),
               dict(cov=not_pd), dict(cov=bad_cov(50.0)), dict(A=2 ** 20 + 1, q=1),
               dict(q=2 ** 16 + 1, A=2 ** 17)]
        for kw in bad:
            o = _outs(4, A)
            assert call(o, **kw) != 0, kw
            assert all(np.all(v == 7) for v in o.values()), kw
        for drop in ("piv", "gain", "zvar0", "rank"):
            o = _outs(4, A)
            keep = dict(o)
            o[drop] = None
            assert call(o) != 0, drop
            assert all(np.all(v == 7) for v in keep.values()), drop
        # the integral: the same rules for the measure, and not all outputs NULL
        m, v, wt = np.full(1, 7.0), np.full(1, 7.0), np.full(n, 7.0)
        for bmu, bcov in ((bad_mu(np.nan), cov), (mu, bad_cov(np.inf)), (mu, not_pd), (None, cov),
                          (mu, None)):
            assert _raw_integral(engine, fit, bmu, bcov, m, v, wt) != 0
            assert m[0] == 7 and v[0] == 7 and np.all(wt == 7)
        assert _raw_integral(engine, fit, mu, cov, None, None, None) != 0
        assert _raw_integral(engine, fit, mu, cov, None, v, None) == 0 and v[0] != 7
        assert _raw_integral(engine, fit, mu, cov, m, None, None) == 0 and m[0] != 7
        assert _raw_integral(engine, fit, mu, cov, None, None, wt) == 0 and np.all(wt != 7)
        assert (m[0], v[0]) == fit.integral(mu, cov)
        for bmu, bcov in ((bad_mu(np.nan), cov), (mu, not_pd)):
            with pytest.raises(ValueError):
                fit.integral(bmu, bcov)
            with pytest.raises(ValueError):
                fit.integral_design(xc, 2, bmu, bcov)
        with pytest.raises(ValueError):
            fit.integral_design(xc, A + 1, mu, cov)
        with pytest.raises(ValueError):
            fit.integral_design(np.zeros((3, 4)), 2, mu, cov)
        # A = 0: rank 0, the tails and zvar0, nothing else touched
        o = _outs(4, A)
        assert call(o, A=0, xc=None) == 0
        assert o["rank"][0] == 0 and np.all(o["piv"] == -1) and np.all(o["gain"] == 0.0)
        assert o["zvar0"][0] == v[0]
        assert np.all(o["ru"] == 7.0) and np.all(o["rc"] == 7.0) and np.all(o["s0"] == 7.0)
        # optional outputs may be missing
        want = fit.integral_design(xc, 4, mu, cov, want_scores=True)
        o = _outs(4, A)
        o.update(ru=None, rc=None, s0=None)
        assert call(o) == 0
        assert o["rank"][0] == 4 and np.array_equal(o["piv"], want[0])
        assert np.array_equal(o["gain"], want[1]) and o["zvar0"][0] == want[2]
        # a single step over a single candidate
        one = fit.integral_design(np.asfortranarray(xc[:, :1]), 1, mu, cov, nugget=s * s,
                                  want_scores=True)
        assert list(one[0]) == [0] and one[1][0] == one[5][0] > 0
        # the fit is not disturbed
        assert np.all(np.isfinite(fit.predict(xc)[1]))
    finally:
        fit.close()


@pytest.mark.parametrize("noisy", [False, True])
def test_larger_launch_shapes(engine, oracle, noisy):
    """The sizes at which the launches take another shape: 256-row workgroups of the product from
    Ap = 16384 on, with more candidates than the picking workgroup has threads' worth of one
    block.  Sigma(xc, xc) does not fit a test: the recurrence needs the columns of it at the
    pivots, the diagonal and u0, all from the definition in long double, the tolerance measured on
    the same pieces by the device's algebra in float64 along the device's pivots.  Held to the
    values, the telescoping sum and greedy-within-tolerance, not to exact pivots."""
    from scipy.linalg import solve_triangular
    n, d, s, A, scale, q = 40, 2, 0.3, 16500, 1.0, 6
    x, y, h, w, s, xc = _case(n, d, s, A, scale)
    mu, cov = _measure(d)
    nu = _nu(s, noisy)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        dev = fit.integral_design(xc, q, mu, cov, nugget=nu, want_scores=True)
        half = fit.integral_design(xc, q // 2, mu, cov, nugget=nu)
        var = fit.predict(xc)[1]
        none = fit.integral_design(xc, 1, mu, cov, tol=1e6)
    finally:
        fit.close()
    piv, gain, zvar0, ru, rc, s0 = dev
    assert piv.shape == (q,) and ru.shape == (A,) and rc.shape == (A,) and s0.shape == (A,)
    assert np.array_equal(half[0], piv[:q // 2]) and np.array_equal(half[1], gain[:q // 2])
    assert np.array_equal(none[4], var)
    xcP = np.asfortranarray(xc[:, piv])
    # long double, from the definition
    Am = _ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD)
    Kcx = _ld_gram(xc, x, h, w)
    Zc = _ld_solve_spd(Am, Kcx.T)
    kx = _ld_kappa(x, h, w, mu, cov)
    om = _ld_solve_spd(Am, kx)
    k0 = _ld_gram(xc[:, :1], xc[:, :1], h, w)[0, 0]
    kk = _ld_kappa(None, h, w, mu, cov, 2)
    ld_in = (_ld_gram(xc, xcP, h, w) - Kcx @ Zc[:, piv], k0 - np.sum(Kcx * Zc.T, axis=1),
             _ld_kappa(xc, h, w, mu, cov) - Kcx @ om, kk - kx @ om)
    # float64, by the device's algebra
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    V = solve_triangular(Lc, np.ascontiguousarray(oracle.gram_cross(x, xc, h, w)), lower=True).T
    b = solve_triangular(Lc, oracle.int_K(x, h, w, mu, cov), lower=True)
    k064 = float(np.asarray(oracle.gram(xc[:, :1], h, w, 0.0))[0, 0])
    vv = np.sum(V * V, axis=1)
    kc64 = oracle.int_K(xc, h, w, mu, cov)
    kk64 = oracle.int_int_K(d, h, w, mu, cov)
    f_in = (np.asarray(oracle.gram_cross(xc, xcP, h, w)) - V @ V[piv].T, k064 - vv, kc64 - V @ b,
            kk64 - b @ b)
    T = k064 + float(vv.max())
    U = float(np.max(kc64) + np.sqrt(vv.max()) * np.linalg.norm(b))
    Zs = float(kk64 + b @ b)

    def along(SP, dc0, u0, z0):
        dt = SP.dtype
        u, dc = u0.copy(), dc0.copy()
        Cf = np.zeros((A, q), dtype=dt)
        taken = np.zeros(A, dtype=bool)
        out = {"scores": [], "gain": [], "zvar": [z0], "den2": []}
        for t, p in enumerate(piv):
            den2 = dc + dt.type(nu)
            ok = (den2 > 0) & ~taken if nu == 0 else den2 > 0
            sc = np.full(A, -np.inf, dtype=dt)
            sc[ok] = u[ok] * u[ok] / den2[ok]
            out["scores"].append(sc), out["gain"].append(sc[p]), out["den2"].append(den2[ok].min())
            den = np.sqrt(den2[p])
            c = (SP[:, t] - Cf[:, :t] @ Cf[p, :t]) / den
            coef = u[p] / den
            if nu == 0:
                c[taken] = 0
                c[p] = den
                taken[p] = True
            u, dc = u - c * coef, dc - c * c
            if nu == 0:
                dc[taken] = 0
                u[taken] = 0
            Cf[:, t] = c
            out["zvar"].append(out["zvar"][-1] - sc[p])
        out["gain"] = np.array(out["gain"], dtype=dt)
        out["u"], out["dc"] = u, dc
        return out

    ld, f64 = along(*ld_in), along(*f_in)
    G = U * U / float(min(ld["den2"]))
    s64 = np.where(np.isfinite(f64["scores"][0]), f64["scores"][0], 0)
    eg, ez, eu, ev = _errors((piv, f64["gain"], f64["zvar"][0], f64["u"], f64["dc"], s64), ld)
    r = max(eg / G, ez / Zs, eu / U, ev / T, float(np.max(np.abs(f_in[0] - ld_in[0]))) / T)
    m = MARGIN * max(r, 4 * EPS)
    tg, tz, tu, tv = m * G, m * Zs, m * U, m * T
    eg, ez, eu, ev = _errors(dev, ld)
    short = max(float(np.max(sc) - sc[p]) for sc, p in zip(ld["scores"], piv))
    tele = abs(float(zvar0 - float(np.sum(gain)) - ld["zvar"][-1]))
    print("A=%d nu=%g: r %.3g; gain error / tol %.3g, var Z error / tol %.3g, u error / tol %.3g, "
          "variance error / tol %.3g, greedy shortfall / tol %.3g, telescoping / tol %.3g"
          % (A, nu, r, eg / tg, ez / tz, eu / tu, ev / tv, short / tg, tele / (tz + q * tg)))
    assert eg <= tg and ez <= tz and eu <= tu and ev <= tv and short <= tg
    assert tele <= tz + q * tg
    if nu == 0.0:
        assert len(set(piv.tolist())) == q and np.all(rc[piv] == 0.0) and np.all(ru[piv] == 0.0)
