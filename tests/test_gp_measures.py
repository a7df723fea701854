"""The kernel means, the integral of a resident fit and its designs under the uniform measure on a
box and under a mixture of Gaussians, on the device (bq_int_K_box, bq_int_K_mix, bq_gp_integral_box,
bq_gp_integral_mix, bq_gp_zdesign_box, bq_gp_zdesign_mix; engine.Engine.int_K_box / int_K_mix and
engine.Fit.integral / integral_design with a ``measures`` object).

* Per entry: kappa and kk for every family and dimension of ld_measures.py at the 256-thread
  workgroup's seams, n in {1, 255, 257}, held to MARGIN max(r, 4 eps) in ld_closed_forms' units, r
  the float64 yardstick's error against the reference -- never the device's.
* The recurrence: four of test_gp_zdesign.py's CASES with its ``_along``, ``_points`` and
  ``_sigma``, the long-double kappa swapped for the box's (mpmath) and the mixture's; the same bars
  (100 max(r, 4 eps) times that file's scales, r from ``numpy_zdesign`` on the oracle's algebra
  with the float64 yardstick for kappa) and the same preconditions on the reference alone.  The box
  covers the middle half of the candidates' range on every axis, so candidates lie inside, on the
  edge and outside; the mixture has three components, one of them off the data.
* Same bits: a mixture with C = 1 and pi = 1 is the Gaussian call, bit for bit, in every output;
  prefixes; repeats.
* State: Gaussian, box, mixture, Gaussian again; the box [0, 1] against the Gaussian (0, 1) in one
  dimension; set_y keeps the state, append and remove recompute it -- each against a fresh fit.

The guard bands of a fit's buffers cannot be read back: bq_plan_check_guards covers the buffers of
a plan (as test_gp_pivchol.py and test_gp_sqwarp.py note), so the largest mixture (64 components,
A = 70) is held to the long-double reference under bq_set_guard(1) and no band is read."""
import functools

import numpy as np
import pytest

import ld_measures as lm
from ld_closed_forms import EPS, LD, MARGIN
from test_gp_fit_state import D, H, S, W, X, XO, Y, Y2
from test_gp_pivchol import _ld_solve_spd
from test_gp_sample import _case, _ld_gram
from test_gp_zdesign import (CASES, LEAD, _along, _errors, _measure, _nu, _points, _sigma,
                             _tolerance)
from test_gp_zdesign_host import numpy_zdesign

pytestmark = pytest.mark.gpu


def _measures():
    from bayesian_quadrature_amd import measures
    return measures


def _box(c):
    return _measures().BoxMeasure(c["lo"], c["hi"])


def _mix(c):
    return _measures().GaussianMixture(c["pi"], c["mu"], c["cov"])


# ---- per entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,d", [(f, d) for f in lm.BOX_FAMILIES for d in lm.box_dims(f)])
def test_box_kernel_mean_per_entry(engine, fam, d):
    worst = 0.0
    for n in lm.SIZES:
        c = lm.box_case(fam, d, n)
        assert lm.all_normal(c["ref"])
        got, kk = engine.int_K_box(c["x"], c["h"], c["w"], _box(c), want_kk=True)
        again = engine.int_K_box(c["x"], c["h"], c["w"], _box(c))
        assert np.array_equal(got, again)
        worst = max(worst, lm.check_kappa(got, c, "box %s d=%d n=%d" % (fam, d, n)))
        wk = lm.check_kk(kk, c, "box %s d=%d" % (fam, d))
    print("box %s d=%d: r %.3g eps, worst kappa error / bar %.3g; r_kk %.3g eps, kk error / bar %.3g"
          % (fam, d, c["r"] / EPS, worst, c["r_kk"] / EPS, wk))


@pytest.mark.parametrize("fam,d", [(f, d) for f in lm.MIX_FAMILIES for d in lm.DIMS])
def test_mixture_kernel_mean_per_entry(engine, fam, d):
    worst = 0.0
    for n in lm.SIZES:
        c = lm.mix_case(fam, d, n)
        assert lm.all_normal(c["ref"])
        got, kk = engine.int_K_mix(c["x"], c["h"], c["w"], _mix(c), want_kk=True)
        worst = max(worst, lm.check_kappa(got, c, "mix %s d=%d n=%d" % (fam, d, n)))
        wk = lm.check_kk(kk, c, "mix %s d=%d" % (fam, d))
    print("mix %s d=%d: r %.3g eps, worst kappa error / bar %.3g; r_kk %.3g eps, kk error / bar %.3g"
          % (fam, d, c["r"] / EPS, worst, c["r_kk"] / EPS, wk))
    if fam == "corr1":  # one component: pi times the Gaussian entry point's bits
        w, pi, mu, cov = lm.mix_params(fam, d)
        one = _measures().GaussianMixture([1.0], mu, cov)
        k1, kk1 = engine.int_K_mix(c["x"], c["h"], w, one, want_kk=True)
        assert np.array_equal(k1, engine.int_K(c["x"], c["h"], w, mu[0], cov[0]))


# ---- the recurrence -------------------------------------------------------------------------------
REC = [c for c in CASES if (c[0], c[1]) in ((65, 1), (130, 3)) or (c[0], c[1], c[3]) == (70, 2, 1)]
assert len(REC) == 4
# (candidates of a seed of their own where _case's do not meet the preconditions on the reference,
# as test_gp_zdesign.py's CASES do it: {(kind, n, d, noisy): seed}.  With _case's candidates the
# d = 1 case leads by 225 (box) and 221 (mixture) tolerances at its closest step, short of LEAD;
# seed 8 is the one of 1 .. 14 with the widest margins on the reference for both measures: 6.0e3
# and 1.5e4 tolerances, dc + nugget of at least 3.6e-3 k0.)
RESEED = {("box", 65, 1, True): 8, ("mix", 65, 1, True): 8}
XC_HALF = 1.65   # the candidates are uniform on [-3.3, 3.3]^d


def _rec_measure(kind, d):
    """(the measure object, ld kappa(pts), ld kk, f64 kappa(pts), f64 kk) for kernel (h, w)."""
    if kind == "box":
        lo, hi = -XC_HALF * np.ones(d), XC_HALF * np.ones(d)
        return (_measures().BoxMeasure(lo, hi),
                lambda p, h, w: lm.mp_box_kappa(p, h, w, lo, hi),
                lambda h, w: lm.mp_box_kk(h, w, lo, hi),
                lambda p, h, w: lm.f64_box_kappa(p, h, w, lo, hi),
                lambda h, w: lm.f64_box_kk(h, w, lo, hi))
    mu0, cov0 = _measure(d)
    pi = np.array([0.5, 0.3, 0.4])
    mu = np.array([mu0, mu0 + 1.2, np.full(d, 4.5)])   # the last one off the data
    cov = np.array([cov0 / 4.0, cov0 / 9.0, 0.25 * np.eye(d)])
    return (_measures().GaussianMixture(pi, mu, cov),
            lambda p, h, w: lm.ld_mix_kappa(p, h, w, pi, mu, cov),
            lambda h, w: lm.ld_mix_kk(h, w, pi, mu, cov),
            lambda p, h, w: lm.f64_mix_kappa(p, h, w, pi, mu, cov),
            lambda h, w: lm.f64_mix_kk(h, w, pi, mu, cov))


@functools.lru_cache(maxsize=None)
def _pieces(oracle, kind, n, d, s, A, scale, seed):
    """test_gp_zdesign._pieces with the measure's kappa and kk."""
    from scipy.linalg import solve_triangular
    x, y, h, w, s, xc = _points(n, d, s, A, scale, seed)
    _, ldk, ldkk, f64k, f64kk = _rec_measure(kind, d)
    sig, T, k0, cpu = _sigma(oracle, n, d, s, A, scale, seed)
    Am = _ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD)
    kx, kc, kk = ldk(x, h, w), ldk(xc, h, w), ldkk(h, w)
    om = _ld_solve_spd(Am, kx)
    ld = dict(kk=kk, weights=om, u0=kc - _ld_gram(xc, x, h, w) @ om, zvar0=kk - kx @ om,
              mean=y.astype(LD) @ om)
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    V = solve_triangular(Lc, np.ascontiguousarray(oracle.gram_cross(x, xc, h, w)), lower=True).T
    b = solve_triangular(Lc, f64k(x, h, w), lower=True)
    z = solve_triangular(Lc, y, lower=True)
    kc64, kk64 = f64k(xc, h, w), float(f64kk(h, w))
    f64 = dict(kk=kk64, weights=solve_triangular(Lc.T, b, lower=False), u0=kc64 - V @ b,
               zvar0=kk64 - b @ b, mean=b @ z)
    vn = np.sqrt(np.max(np.sum(V * V, axis=1)))
    return dict(ld=ld, f64=f64, T=T, k0=k0, sig=sig, cpu=cpu,
                U=float(np.max(kc64) + vn * np.linalg.norm(b)), Zs=float(kk64 + b @ b),
                Ms=float(np.linalg.norm(b) * np.linalg.norm(z)))


@functools.lru_cache(maxsize=None)
def _device(engine, kind, n, d, s, A, scale, q, noisy, seed):
    x, y, h, w, s, xc = _points(n, d, s, A, scale, seed)
    m = _rec_measure(kind, d)[0]
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        out = fit.integral_design(xc, q, m, nugget=_nu(s, noisy), want_scores=True)
        integ = fit.integral(m, want_weights=True)
    finally:
        fit.close()
    return out, integ


def _rec_cases():
    return [(kind,) + c[:7] + (RESEED.get((kind, c[0], c[1], c[6]), c[7]),)
            for kind in ("box", "mix") for c in REC]


@pytest.mark.parametrize("kind,n,d,s,A,scale,q,noisy,seed", _rec_cases())
def test_design_holds_its_contract(engine, oracle, kind, n, d, s, A, scale, q, noisy, seed):
    pc = _pieces(oracle, kind, n, d, s, A, scale, seed)
    nu = _nu(s, noisy)
    dev, integ = _device(engine, kind, n, d, s, A, scale, q, noisy, seed)
    piv, gain, zvar0, ru, rc, s0 = dev
    label = "%s n=%d d=%d A=%d q=%d nu=%g" % (kind, n, d, A, q, nu)
    assert piv.shape == (q,) and piv.dtype == np.int64 and gain.shape == (q,)  # full rank
    assert np.all((piv >= 0) & (piv < A)) and np.all(gain > 0)
    assert np.all(np.isfinite(ru)) and np.all(np.isfinite(rc)) and np.all(np.isfinite(s0))
    assert s0[piv[0]] == gain[0] == s0.max() and piv[0] == int(np.argmax(s0))
    ld = _along(pc["sig"], pc["ld"]["u0"], pc["ld"]["zvar0"], piv, nu)
    tg, tz, tu, tv = _tolerance(pc, piv, nu, ld, label)
    eg, ez, eu, ev = _errors(dev, ld)
    short = max(float(np.max(sc) - sc[p]) for sc, p in zip(ld["scores"], piv))
    tele = abs(float(zvar0 - float(np.sum(gain)) - ld["zvar"][-1]))
    print("%s: gain error / tol %.3g, var Z error / tol %.3g, u error / tol %.3g, variance error "
          "/ tol %.3g, greedy shortfall / tol %.3g, telescoping / tol %.3g"
          % (label, eg / tg, ez / tz, eu / tu, ev / tv, short / tg, tele / (tz + q * tg)))
    assert eg <= tg and ez <= tz and eu <= tu and ev <= tv and short <= tg
    assert tele <= tz + q * tg
    if nu == 0.0:
        assert len(set(piv.tolist())) == q and np.all(rc[piv] == 0.0) and np.all(ru[piv] == 0.0)
    else:
        assert np.all(rc > 0)
    # the integral: the design's zvar0 is its var, bit for bit; mean, var and weights against long
    # double with test_gp_zdesign.test_integral_against_long_double's bars
    mean, var, wts = integ
    assert var == zvar0
    f64, l = pc["f64"], pc["ld"]
    Ws = float(np.max(np.abs(f64["weights"])))
    rm = abs(float(f64["mean"] - l["mean"])) / pc["Ms"]
    rz = abs(float(f64["zvar0"] - l["zvar0"])) / pc["Zs"]
    rw = float(np.max(np.abs(f64["weights"] - l["weights"]))) / Ws
    tm, tz2, tw = (MARGIN * max(r, 4 * EPS) * sc for r, sc in ((rm, pc["Ms"]), (rz, pc["Zs"]),
                                                               (rw, Ws)))
    em, ez2 = abs(float(mean - l["mean"])), abs(float(var - l["zvar0"]))
    ew = float(np.max(np.abs(wts - l["weights"])))
    print("%s: integral error / tol mean %.3g var %.3g weights %.3g"
          % (label, em / tm, ez2 / tz2, ew / tw))
    assert em <= tm and ez2 <= tz2 and ew <= tw


@pytest.mark.parametrize("kind,n,d,s,A,scale,q,noisy,seed", _rec_cases())
def test_pivots_are_the_reference_s(engine, oracle, kind, n, d, s, A, scale, q, noisy, seed):
    pc = _pieces(oracle, kind, n, d, s, A, scale, seed)
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
    tg = _tolerance(pc, want, nu, ld, "%s n=%d d=%d A=%d q=%d nu=%g" % (kind, n, d, A, q, nu))[0]
    den2 = float(min(ld["den2"]))
    kk = float(pc["ld"]["kk"])
    print("smallest lead %.3g kk = %.3g tol, smallest dc + nu %.3g k0, smallest gain %.3g kk"
          % (min(leads) / kk, min(leads) / tg, den2 / pc["k0"], float(np.min(wgain)) / kk))
    assert min(leads) >= LEAD * tg
    assert den2 >= 1.5e-3 * pc["k0"]
    piv, gain = _device(engine, kind, n, d, s, A, scale, q, noisy, seed)[0][:2]
    assert np.array_equal(piv, want)
    assert float(np.max(np.abs(gain - wgain.astype(np.float64)))) <= tg


# ---- same bits --------------------------------------------------------------------------------------
def _eq(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b)) and len(a) == len(b)


def test_one_component_is_the_gaussian_call_bit_for_bit(engine):
    n, d, s, A, scale, q = 130, 2, 0.05, 200, 0.5, 5
    x, y, h, w, s, xc = _case(n, d, s, A, scale)
    mu, cov = _measure(d)
    one = _measures().GaussianMixture([1.0], mu[None, :], cov[None, :, :])
    f, g = engine.gp_fit(x, y, h, w, s), engine.gp_fit(x, y, h, w, s)
    try:
        assert _eq(f.integral(one, want_weights=True), g.integral(mu, cov, want_weights=True))
        for nu in (0.0, s * s):
            a = f.integral_design(xc, q, one, nugget=nu, want_scores=True)
            b = g.integral_design(xc, q, mu, cov, nugget=nu, want_scores=True)
            assert len(a[0]) == q and _eq(a, b)
        # the design computes the state on its way: fresh fits, design first
        f2, g2 = engine.gp_fit(x, y, h, w, s), engine.gp_fit(x, y, h, w, s)
        try:
            assert _eq(f2.integral_design(xc, q, one, want_scores=True),
                       g2.integral_design(xc, q, mu, cov, want_scores=True))
        finally:
            f2.close(), g2.close()
        # on one fit the two are two keys of one state, and each keeps its bits
        assert _eq(f.integral(mu, cov, want_weights=True), f.integral(one, want_weights=True))
        assert np.array_equal(engine.int_K_mix(xc, h, w, one), engine.int_K(xc, h, w, mu, cov))
    finally:
        f.close(), g.close()


def test_box_design_prefixes_and_repeats(engine):
    n, d, s, A, scale, q = 130, 2, 0.05, 200, 0.5, 12
    x, y, h, w, s, xc = _case(n, d, s, A, scale)
    box = _rec_measure("box", d)[0]
    mix = _rec_measure("mix", d)[0]
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        for m in (box, mix):
            for nu in (0.0, s * s):
                full = fit.integral_design(xc, q, m, nugget=nu, want_scores=True)
                assert _eq(full, fit.integral_design(xc, q, m, nugget=nu, want_scores=True))
                for j in (1, 5, q):
                    part = fit.integral_design(xc, j, m, nugget=nu, want_scores=True)
                    assert np.array_equal(part[0], full[0][:j])
                    assert np.array_equal(part[1], full[1][:j])
                    assert part[2] == full[2] and np.array_equal(part[5], full[5])
            a = fit.integral(m, want_weights=True)
            assert _eq(a, fit.integral(m, want_weights=True)) and a[1] == full[2]
        # no candidates: zvar0 alone
        e = fit.integral_design(np.empty((d, 0)), 3, box)
        assert e[0].shape == (0,) and e[2] == fit.integral(box)[1]
    finally:
        fit.close()


# ---- state ------------------------------------------------------------------------------------------
def _state_measures():
    ms = _measures()
    gauss = (np.array([0.4, -0.3]), np.array([[1.0, 0.3], [0.3, 0.8]]))
    box = ms.BoxMeasure([-1.5, -2.0], [2.0, 1.0])
    mix = ms.GaussianMixture([0.6, 0.4], [[1.0, 0.5], [-1.5, 0.2]],
                             [[[0.5, 0.1], [0.1, 0.4]], [[0.0, 0.0], [0.0, 0.0]]])
    return gauss, box, mix


def _ask(f, m):
    return f.integral(*m, want_weights=True) if isinstance(m, tuple) \
        else f.integral(m, want_weights=True)


def test_keyed_state_follows_the_measure_s_kind(engine):
    n = 130
    x, y = np.asfortranarray(X[:, :n]), Y[:n]
    gauss, box, mix = _state_measures()
    f = engine.gp_fit(x, y, H, W, S)
    try:
        first = [_ask(f, m) for m in (gauss, box, mix)]
        assert _eq(_ask(f, gauss), first[0])
        assert _eq(_ask(f, mix), first[2]) and _eq(_ask(f, box), first[1])
        for m, a in zip((gauss, box, mix), first):
            g = engine.gp_fit(x, y, H, W, S)
            try:
                assert _eq(_ask(g, m), a)
            finally:
                g.close()
        assert first[0][1] != first[1][1] != first[2][1]
    finally:
        f.close()


def test_a_box_and_a_gaussian_with_the_same_numbers_do_not_share_state(engine):
    ms = _measures()
    rs = np.random.RandomState(3)
    x, y = np.sort(rs.uniform(-2, 3, 70)), rs.randn(70)
    box = ms.BoxMeasure([0.0], [1.0])
    f = engine.gp_fit(x, y, 1.1, [0.4], 0.1)
    g, b = engine.gp_fit(x, y, 1.1, [0.4], 0.1), engine.gp_fit(x, y, 1.1, [0.4], 0.1)
    try:
        a1 = f.integral([0.0], [[1.0]], want_weights=True)
        a2 = f.integral(box, want_weights=True)
        a3 = f.integral([0.0], [[1.0]], want_weights=True)
        assert a1[0] != a2[0] and a1[1] != a2[1] and not np.array_equal(a1[2], a2[2])
        assert _eq(a1, a3)
        assert _eq(a1, g.integral([0.0], [[1.0]], want_weights=True))
        assert _eq(a2, b.integral(box, want_weights=True))
    finally:
        f.close(), g.close(), b.close()


def test_state_survives_new_targets_and_follows_the_factor(engine):
    n = 130
    x, y, y2 = np.asfortranarray(X[:, :n]), Y[:n], Y2[:n]
    _, box, mix = _state_measures()
    rs = np.random.RandomState(11)
    xn, yn = np.asfortranarray(rs.uniform(-3, 3, size=(D, 5))), rs.randn(5)
    for m in (box, mix):
        warm = engine.gp_fit(x, y, H, W, S)
        try:
            before = _ask(warm, m)
            warm.set_y(y2), warm.refit(H, W, S)
            after = _ask(warm, m)
            fresh = engine.gp_fit(x, y2, H, W, S)
            try:
                assert _eq(after, _ask(fresh, m))
            finally:
                fresh.close()
            assert after[1] == before[1] and np.array_equal(after[2], before[2])
            assert after[0] != before[0]
            warm.append(xn, yn)
            cold = engine.gp_fit(x, y2, H, W, S)
            try:
                cold.append(xn, yn)
                a = _ask(warm, m)
                assert _eq(a, _ask(cold, m)) and a[1] != after[1]
                idx = np.array([3, 64, 100])
                warm.remove(idx), cold.remove(idx)
                r = _ask(warm, m)
                assert _eq(r, _ask(cold, m)) and r[1] != a[1]
                da = warm.integral_design(XO, 4, m)
                assert _eq(da, cold.integral_design(XO, 4, m))
            finally:
                cold.close()
        finally:
            warm.close()


def test_the_largest_mixture_under_guard_bands(engine, oracle):
    """64 components, A = 70, every buffer allocated with its guard band (bq_set_guard(1)): the
    design's first score vector, zvar0 and the integral against long double."""
    n, d, s, A, scale = 70, 2, 0.05, 70, 0.5
    x, y, h, w, s, xc = _points(n, d, s, A, scale, None)
    rs = np.random.RandomState(64)
    pi, mu = rs.uniform(0.0, 1.0, 64), rs.uniform(-3.0, 3.0, (64, d))
    cov = np.array([sc * sc * np.eye(d) for sc in rs.uniform(0.0, 1.0, 64)])
    cov[::7] = 0.0
    m = _measures().GaussianMixture(pi, mu, cov)
    engine.set_guard(True)
    try:
        fit = engine.gp_fit(x, y, h, w, s)
        try:
            piv, gain, zvar0, ru, rc, s0 = fit.integral_design(xc, 9, m, nugget=s * s,
                                                               want_scores=True)
            mean, var, wts = fit.integral(m, want_weights=True)
        finally:
            fit.close()
    finally:
        engine.set_guard(False)
    Am = _ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD)
    kx, kc = lm.ld_mix_kappa(x, h, w, pi, mu, cov), lm.ld_mix_kappa(xc, h, w, pi, mu, cov)
    kk = lm.ld_mix_kk(h, w, pi, mu, cov)
    om = _ld_solve_spd(Am, kx)
    sig = _sigma(oracle, n, d, s, A, scale, None)[0]
    ld = _along(sig, kc - _ld_gram(xc, x, h, w) @ om, kk - kx @ om, piv, s * s)
    # the float64 yardstick by the oracle's algebra gives r, as above
    from scipy.linalg import solve_triangular
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    b = solve_triangular(Lc, lm.f64_mix_kappa(x, h, w, pi, mu, cov), lower=True)
    kk64 = float(lm.f64_mix_kk(h, w, pi, mu, cov))
    Zs = kk64 + b @ b
    r = abs(float((kk64 - b @ b) - ld["zvar"][0])) / Zs
    tz = MARGIN * max(r, 4 * EPS) * Zs
    print("64 components: r %.3g, var Z error / tol %.3g" % (r, abs(float(var - ld["zvar"][0])) / tz))
    assert len(piv) == 9 and var == zvar0 and abs(float(var - ld["zvar"][0])) <= tz
    assert np.isfinite(mean) and wts.shape == (n,)


# ---- argument errors ---------------------------------------------------------------------------------
def test_argument_errors_write_nothing(engine):
    """Every illegal measure of include/bqhip.h through the C entry points: a status that is not
    0, and no output touched."""
    import ctypes as C
    from test_gp_zdesign import _outs
    x, y, h, w, s, xc = _case(40, 2, 0.3, 10, 1.0)
    A, n, d = 10, 40, 2
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def p(a, t=dp):
        return None if a is None else a.ctypes.data_as(t)   # (every array here is contiguous)

    lo, hi = np.array([-1.0, -2.0]), np.array([1.0, 0.5])
    pi, mu = np.array([0.5, 0.5]), np.array([[0.0, 1.0], [1.0, -1.0]])
    cov = np.array([np.eye(2), np.zeros((2, 2))])

    def edit(a, idx, v):
        b = np.array(a, dtype=np.float64)
        b[idx] = v
        return b

    bad_box = [(None, hi), (lo, None), (edit(lo, 1, np.nan), hi), (lo, edit(hi, 0, np.inf)),
               (lo, edit(hi, 1, -2.0)), (lo, edit(hi, 1, -3.0))]          # lo == hi, lo > hi
    bad_mix = [(2, None, mu, cov), (2, pi, None, cov), (2, pi, mu, None), (0, pi, mu, cov),
               (-1, pi, mu, cov), (65, np.ones(65), np.zeros((65, 2)), np.zeros((65, 2, 2))),
               (2, edit(pi, 0, np.nan), mu, cov), (2, pi, edit(mu, (1, 0), np.inf), cov),
               (2, pi, mu, edit(cov, (0, 0, 1), np.nan)), (2, edit(pi, 1, -0.1), mu, cov),
               (2, np.zeros(2), mu, cov),
               (2, pi, mu, edit(cov, (0, 0, 0), -10.0)),                   # W + Sigma_0 fails
               (2, pi, mu, np.array([-0.6 * np.diag(w ** 2)] * 2))]        # only W + S_c + S_c' fails
    lib, ctx = engine._lib, engine._ctx
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        fh = fit._handle()
        for args, name in [((p(a), p(b)), "_box") for a, b in bad_box] + \
                [((c, p(a), p(b), p(v)), "_mix") for c, a, b, v in bad_mix]:
            m, v, wt = np.full(1, 7.0), np.full(1, 7.0), np.full(n, 7.0)
            st = getattr(lib, "bq_gp_integral" + name)(ctx, fh, *args, p(m), p(v), p(wt))
            assert st != 0 and m[0] == 7 and v[0] == 7 and np.all(wt == 7), (name, args)
            o = _outs(4, A)
            st = getattr(lib, "bq_gp_zdesign" + name)(
                ctx, fh, *args, p(xc), A, 4, 0.0, 0.0, p(o["piv"], ip), p(o["gain"]),
                p(o["zvar0"]), p(o["ru"]), p(o["rc"]), p(o["s0"]), p(o["rank"], ip))
            assert st != 0 and all(np.all(a == 7) for a in o.values()), (name, args)
            out, kk = np.full(n, 7.0), np.full(1, 7.0)
            st = getattr(lib, "bq_int_K" + name)(ctx, p(x), d, n, h, p(w), *args, p(out), p(kk))
            assert st != 0 and np.all(out == 7) and kk[0] == 7, (name, args)
        # both outputs NULL; zd_args' rules with a legal measure; A == 0
        assert lib.bq_int_K_box(ctx, p(x), d, n, h, p(w), p(lo), p(hi), None, None) != 0
        assert lib.bq_gp_integral_box(ctx, fh, p(lo), p(hi), None, None, None) != 0
        o = _outs(4, A)
        assert lib.bq_gp_zdesign_box(ctx, fh, p(lo), p(hi), p(xc), A, A + 1, 0.0, 0.0,
                                     p(o["piv"], ip), p(o["gain"]), p(o["zvar0"]), p(o["ru"]),
                                     p(o["rc"]), p(o["s0"]), p(o["rank"], ip)) != 0
        assert all(np.all(a == 7) for a in o.values())
        ms = _measures()
        box = ms.BoxMeasure(lo, hi)
        assert lib.bq_gp_zdesign_box(ctx, fh, p(lo), p(hi), None, 0, 4, 0.0, 0.0,
                                     p(o["piv"], ip), p(o["gain"]), p(o["zvar0"]), p(o["ru"]),
                                     p(o["rc"]), p(o["s0"]), p(o["rank"], ip)) == 0
        assert o["rank"][0] == 0 and np.all(o["piv"] == -1) and np.all(o["gain"] == 0.0)
        assert o["zvar0"][0] == fit.integral(box)[1] and np.all(o["ru"] == 7.0)
        # either output alone; kk needs no points
        kap, kk = engine.int_K_box(x, h, w, box, want_kk=True)
        kk1 = np.full(1, 7.0)
        assert lib.bq_int_K_box(ctx, None, d, 0, h, p(w), p(lo), p(hi), None, p(kk1)) == 0
        assert kk1[0] == kk
        with pytest.raises(ValueError):
            fit.integral(ms.GaussianMixture([1.0], [[0.0, 0.0]], [-10.0 * np.eye(2)]))
        # the fit is not disturbed
        assert np.all(np.isfinite(fit.predict(xc)[1]))
    finally:
        fit.close()
