"""Square-root-warped Bayesian quadrature of a resident fit on the device (bq_gp_sqintegral,
bq_gp_sqdesign; engine.Fit.sq_integral, engine.Fit.sq_integral_design) against explicit CPU
references.

Cases, points and the measure are test_gp_zdesign.py's; the targets are g = sqrt(2 (l - alpha0))
of the positive function l(x) = exp(-|x|^2 / (2 1.5^2)) + 0.05 at the fit's points, alpha0 =
0.8 min l.  The references are in long double: the closed forms of test_gp_sqwarp_host.py (W, Q),
test_gp_pivchol._ld_solve_spd, and the recurrence of include/bqhip.h along the device's own pivots
(test_gp_zdesign._along).

The pair sums run with one column slice where the fit has at most 128 points (n = 65 and 70: one
tile of BQ_SQ_TJ columns) and with two where it has more (n = 130 and 200); the row blocks (256
rows) are one (A <= 256, n <= 256) or two (A = 330), the last one partly filled in every case.

The tolerances are measured, as in test_gp_zdesign.py: the float64 restatement
(test_gp_sqwarp_host.numpy_sqintegral, numpy_squ0, test_gp_zdesign_host.numpy_zdesign) runs on the
oracle's algebra -- its Gram, Cholesky, triangular solve, int_K1_K2, int_int_K1_K2_K1 and
K - V V^T -- along the device's pivots, and its largest error against long double gives r relative
to the size of the terms: sum_ij |alpha_i| W_ij |alpha_j| for sq, max_i sum_j W_ij |alpha_j| for r,
qq + |b_w|^2 for the variance, U = max |kap| + max_a ||v_a|| |b_w| for u, U^2 over the smallest
eligible dc + nugget for scores and gains, T = max diag K + max_a ||v_a||^2 for the variances
left.  The device gets 100 max(r, 4 eps) times that scale.

BQ_GUARD and bq_plan_check_guards cover the buffers of a plan, not those of a fit, so there is no
guard-band test here (as in test_gp_pivchol.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gp_pivchol import _ld_solve_spd
from test_gp_sample import _case, _ld_gram
from test_gp_sqwarp_host import Q_closed, W_closed, numpy_sqintegral, numpy_squ0
from test_gp_zdesign import (CASES, EPS, LD, LEAD, MARGIN, _along, _errors, _measure, _nu, _points,
                             _sigma)
from test_gp_zdesign_host import numpy_zdesign

pytestmark = pytest.mark.gpu

# test_gp_zdesign.py's cases, (n, d, s, A, w scale, q, noisy, seed).  Two of them draw their
# candidates from a seed of their own, RandomState(seed).uniform(-3.3, 3.3), as one of that file's
# does: with these targets and _case's candidates, (130, 2, 0.05, 70) with a nugget leads by only
# 446 tolerances at its closest step (LEAD asks 1000), and (70, 2, 0.05, 63) without one has a
# smallest eligible dc of 2.1e-4 k0 (1.5e-3 k0 is asked).  Of the seeds 1 .. 20, 1 gives the first
# a lead of 5.4e3 tolerances and dc + nugget of at least 2.0e-3 k0, 11 gives the second a lead of
# 2.9e6 tolerances and dc of at least 7.7e-3 k0 -- figures from the long-double reference alone.
assert CASES[3] == (130, 2, 0.05, 70, 0.5, 32, True, None)
assert CASES[7] == (70, 2, 0.05, 63, 0.5, 9, False, None)
SQ_CASES = CASES[:3] + [CASES[3][:7] + (1,)] + CASES[4:7] + [CASES[7][:7] + (11,)] + CASES[8:]


def _targets(x):
    l = np.exp(-0.5 * np.sum(x * x, axis=0) / 1.5 ** 2) + 0.05
    return np.sqrt(2.0 * (l - 0.8 * l.min()))


@functools.lru_cache(maxsize=None)
def _pieces(oracle, n, d, s, A, scale, seed=None):
    """What the tests of a case share: {"ld": alpha, r, sq, qq, var, u0 in long double; "f64": the
    same by the oracle's algebra in float64; the scales; sig, cpu, k0, T of test_gp_zdesign}."""
    from scipy.linalg import solve_triangular
    x, _, h, w, s, xc = _points(n, d, s, A, scale, seed)
    y = _targets(x)
    mu, cov = _measure(d)
    sig, T, k0, cpu = _sigma(oracle, n, d, s, A, scale, seed)
    xl, cl = x.astype(LD), xc.astype(LD)
    Am = _ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD)
    al = _ld_solve_spd(Am, y.astype(LD))
    Wl = W_closed(xl, xl, h, w, mu, cov)
    rl = Wl @ al
    om = _ld_solve_spd(Am, rl)
    qql = al @ Q_closed(xl, h, w, mu, cov) @ al
    ld = dict(alpha=al, r=rl, sq=al @ rl, qq=qql, zvar0=qql - rl @ om,
              u0=W_closed(cl, xl, h, w, mu, cov) @ al - _ld_gram(xc, x, h, w) @ om)
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    V = solve_triangular(Lc, np.ascontiguousarray(oracle.gram_cross(x, xc, h, w)), lower=True).T
    a64 = solve_triangular(Lc.T, solve_triangular(Lc, y, lower=True), lower=False)
    W64 = np.asarray(oracle.int_K1_K2(x, x, h, w, h, w, mu, cov))
    Q64 = np.asarray(oracle.int_int_K1_K2_K1(x, h, w, h, w, mu, cov))
    r64 = W64 @ a64
    b64 = solve_triangular(Lc, r64, lower=True)
    kc64 = np.asarray(oracle.int_K1_K2(xc, x, h, w, h, w, mu, cov)) @ a64
    qq64 = a64 @ Q64 @ a64
    f64 = dict(alpha=a64, r=r64, sq=a64 @ r64, qq=qq64, zvar0=qq64 - b64 @ b64, u0=kc64 - V @ b64)
    vn = np.sqrt(np.max(np.sum(V * V, axis=1)))
    out = dict(ld=ld, f64=f64, T=T, k0=k0, sig=sig, cpu=cpu, y=y,
               Ss=float(np.abs(a64) @ W64 @ np.abs(a64)), Rs=float(np.max(W64 @ np.abs(a64))),
               Zs=float(qq64 + b64 @ b64),
               U=float(np.max(np.abs(kc64)) + vn * np.linalg.norm(b64)))
    for v in list(ld.values()) + list(f64.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _tolerance(pc, piv, nu, ld, label):
    """(tol for gains and scores, for var Z, for u, for variances, for sq, for r): 100 max(r, 4 eps)
    times the scales of the module docstring, r from the float64 restatement on the oracle's
    algebra along the device's pivots."""
    f64, T, U, Zs = pc["f64"], pc["T"], pc["U"], pc["Zs"]
    G = U * U / float(min(ld["den2"])) if len(piv) else U * U / pc["k0"]
    r = max(float(np.max(np.abs(pc["cpu"] - pc["sig"]))) / T,
            float(np.max(np.abs(f64["u0"] - pc["ld"]["u0"]))) / U,
            float(abs(f64["zvar0"] - pc["ld"]["zvar0"])) / Zs,
            float(abs(f64["sq"] - pc["ld"]["sq"])) / pc["Ss"],
            float(np.max(np.abs(f64["r"] - pc["ld"]["r"]))) / pc["Rs"])
    if len(piv):
        out = numpy_zdesign(np.array(pc["cpu"]), f64["u0"], f64["zvar0"], f64["qq"], pc["k0"],
                            len(piv), nu, 0.0, pivots=piv)
        if out[6] == len(piv):
            eg, ez, eu, ev = _errors((piv,) + out[1:6], ld)
            r = max(r, eg / G, ez / Zs, eu / U, ev / T)
    print("%s: r %.3g" % (label, r))
    m = MARGIN * max(r, 4 * EPS)
    return m * G, m * Zs, m * U, m * T, m * pc["Ss"], m * pc["Rs"]


def _fit(engine, n, d, s, A, scale, seed=None):
    x, _, h, w, s, xc = _points(n, d, s, A, scale, seed)
    return engine.gp_fit(x, _targets(x), h, w, s), xc


@functools.lru_cache(maxsize=None)
def _device(engine, n, d, s, A, scale, q, noisy, seed=None):
    mu, cov = _measure(d)
    fit, xc = _fit(engine, n, d, s, A, scale, seed)
    try:
        out = fit.sq_integral_design(xc, q, mu, cov, nugget=_nu(s, noisy), want_scores=True)
    finally:
        fit.close()
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("n,d,s,A,scale,q,noisy,seed", SQ_CASES)
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
    tg, tz, tu, tv = _tolerance(pc, piv, nu, ld, label)[:4]
    eg, ez, eu, ev = _errors(dev, ld)
    short = max(float(np.max(sc) - sc[p]) for sc, p in zip(ld["scores"], piv))
    tele = abs(float(zvar0 - float(np.sum(gain)) - ld["zvar"][-1]))
    print("%s: gain error / tol %.3g, var Z error / tol %.3g, u error / tol %.3g, variance error "
          "/ tol %.3g, greedy shortfall / tol %.3g, telescoping / tol %.3g, smallest gain / qq %.3g"
          % (label, eg / tg, ez / tz, eu / tu, ev / tv, short / tg, tele / (tz + q * tg),
             float(np.min(gain)) / pc["f64"]["qq"]))
    assert eg <= tg and ez <= tz and eu <= tu and ev <= tv and short <= tg
    assert tele <= tz + q * tg
    if nu == 0.0:
        assert len(set(piv.tolist())) == q and np.all(rc[piv] == 0.0) and np.all(ru[piv] == 0.0)
    else:
        assert np.all(rc > 0)


@pytest.mark.parametrize("n,d,s,A,scale,q,noisy,seed", SQ_CASES)
def test_pivots_are_the_reference_s(engine, oracle, n, d, s, A, scale, q, noisy, seed):
    pc = _pieces(oracle, n, d, s, A, scale, seed)
    nu = _nu(s, noisy)
    want, wgain, _, _, _, _, rank = numpy_zdesign(
        pc["sig"].astype(LD), pc["ld"]["u0"], pc["ld"]["zvar0"], pc["ld"]["qq"], LD(pc["k0"]), q,
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
    qq = float(pc["ld"]["qq"])
    print("smallest lead %.3g qq = %.3g tol, smallest dc + nu %.3g k0, smallest gain %.3g qq"
          % (min(leads) / qq, min(leads) / tg, den2 / pc["k0"], float(np.min(wgain)) / qq))
    assert min(leads) >= LEAD * tg
    assert den2 >= 1.5e-3 * pc["k0"]
    piv, gain = _device(engine, n, d, s, A, scale, q, noisy, seed)[:2]
    assert np.array_equal(piv, want)
    assert float(np.max(np.abs(gain - wgain.astype(np.float64)))) <= tg


@pytest.mark.parametrize("n,d,s,A,scale", [(65, 3, 0.1, 64, 1.0), (130, 2, 0.05, 70, 0.5),
                                            (200, 3, 0.1, 330, 1.0), (65, 1, 0.1, 64, 0.25)])
def test_integral_against_long_double(engine, oracle, n, d, s, A, scale):
    pc = _pieces(oracle, n, d, s, A, scale)
    mu, cov = _measure(d)
    ld = pc["ld"]
    fit, xc = _fit(engine, n, d, s, A, scale)
    try:
        sq, var, r = fit.sq_integral(mu, cov, want_r=True)
        again = fit.sq_integral(mu, cov, want_r=True)  # the state is there: the same bits
        assert again[0] == sq and again[1] == var and np.array_equal(again[2], r)
        assert fit.sq_integral(mu, cov) == (sq, var)
        alpha = fit.alpha()
    finally:
        fit.close()
    _, tz, _, _, ts, tr = _tolerance(pc, [], 0.0, None, "n=%d d=%d" % (n, d))
    es, ez = abs(float(sq - ld["sq"])), abs(float(var - ld["zvar0"]))
    er = float(np.max(np.abs(r - ld["r"])))
    print("n=%d d=%d: error / tol sq %.3g var %.3g r %.3g; var / qq %.3g"
          % (n, d, es / ts, ez / tz, er / tr, var / pc["f64"]["qq"]))
    assert r.shape == (n,) and es <= ts and ez <= tz and er <= tr
    assert abs(float(alpha @ r) - sq) <= ts


def test_same_bits_prefixes_and_the_shared_workspaces(engine):
    """Two calls give the same bits; a j-step call is the prefix of a q-step call; the state
    survives calls with the same measure; bq_gp_zdesign on the same fit gives identical bits
    before and after a bq_gp_sqdesign call, and the reverse (they share workspaces)."""
    n, d, s, A, scale, q = 130, 3, 0.1, 200, 1.0, 24
    mu, cov = _measure(d)
    fit, xc = _fit(engine, n, d, s, A, scale)
    try:
        zd0 = fit.integral_design(xc, q, mu, cov, nugget=s * s, want_scores=True)
        first = fit.sq_integral(mu, cov, want_r=True)
        for nu in (0.0, s * s):
            full = fit.sq_integral_design(xc, q, mu, cov, nugget=nu, want_scores=True)
            again = fit.sq_integral_design(xc, q, mu, cov, nugget=nu, want_scores=True)
            assert all(np.array_equal(a, b) for a, b in zip(full, again))
            for j in (1, q // 2, 17, q):
                part = fit.sq_integral_design(xc, j, mu, cov, nugget=nu, want_scores=True)
                assert np.array_equal(part[0], full[0][:j])
                assert np.array_equal(part[1], full[1][:j])
                assert part[2] == full[2] and np.array_equal(part[5], full[5])
            bare = fit.sq_integral_design(xc, q, mu, cov, nugget=nu)
            assert len(bare) == 5 and all(np.array_equal(a, b) for a, b in zip(bare, full))
            assert full[2] == first[1]
        zd1 = fit.integral_design(xc, q, mu, cov, nugget=s * s, want_scores=True)
        assert all(np.array_equal(a, b) for a, b in zip(zd0, zd1))
        sq1 = fit.sq_integral_design(xc, q, mu, cov, nugget=s * s, want_scores=True)
        assert all(np.array_equal(a, b) for a, b in zip(sq1, full))
        last = fit.sq_integral(mu, cov, want_r=True)
        assert last[:2] == first[:2] and np.array_equal(last[2], first[2])
        # the sweep under it is bq_gp_predict's, and a stop level above every gain ends at once
        var = fit.predict(xc)[1]
        p0, g0, zvar0, ru, rc = fit.sq_integral_design(xc, 1, mu, cov, tol=1e6)
        assert p0.shape == (0,) and g0.shape == (0,) and np.array_equal(rc, var)
        assert zvar0 == first[1]
        # a cold fit that goes straight to the design computes the same state on its way
        cold, _ = _fit(engine, n, d, s, A, scale)
        try:
            c = cold.sq_integral_design(xc, q, mu, cov, nugget=s * s, want_scores=True)
            assert all(np.array_equal(a, b) for a, b in zip(c, full))
        finally:
            cold.close()
    finally:
        fit.close()


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_derived_state_follows_the_events(engine):
    """The SQW row of the derived-state table, with twins: a warm fit that has computed the state
    before the event against a cold one that computes it after.  Unlike KMEAN it depends on the
    targets: after set_y it is rebuilt, and equals a fresh fit's on the new targets."""
    n, d, s, A, scale = 130, 3, 0.1, 8, 1.0
    x, _, h, w, s, xc = _case(n, d, s, A, scale)
    y = _targets(x)
    mu, cov = _measure(d)
    mu2, cov2 = mu + 0.5, np.asfortranarray(cov * 0.5)
    y2 = np.sqrt(y * y + 0.3)
    rs = np.random.RandomState(11)
    xn, yn = np.asfortranarray(rs.uniform(-3, 3, size=(d, 5))), rs.uniform(0.1, 1.0, 5)

    def events():
        yield "set_y", lambda f: (f.set_y(y2), f.refit(h, w, s))
        yield "refit", lambda f: f.refit(1.1 * h, 0.9 * w, s)
        yield "append", lambda f: f.append(xn, yn)
        yield "remove", lambda f: f.remove(np.array([3, 64, 100]))

    for name, ev in events():
        warm, cold = engine.gp_fit(x, y, h, w, s), engine.gp_fit(x, y, h, w, s)
        try:
            before = warm.sq_integral(mu, cov, want_r=True)
            ev(warm), ev(cold)
            a = warm.sq_integral(mu, cov, want_r=True)
            b = cold.sq_integral(mu, cov, want_r=True)
            assert _same(a, b), name
            assert a[0] != before[0] and a[1] != before[1], name
            if name == "set_y":
                fresh = engine.gp_fit(x, y2, h, w, s)
                try:
                    assert _same(fresh.sq_integral(mu, cov, want_r=True), a)
                finally:
                    fresh.close()
            da = warm.sq_integral_design(xc, 4, mu2, cov2)
            db = cold.sq_integral_design(xc, 4, mu2, cov2)
            assert all(np.array_equal(u, v) for u, v in zip(da, db)), name
            assert da[2] == warm.sq_integral(mu2, cov2)[1]
        finally:
            warm.close(), cold.close()
    # a second key recomputes; going back gives the first bits; KMEAN keeps its own key
    f = engine.gp_fit(x, y, h, w, s)
    try:
        a = f.sq_integral(mu, cov, want_r=True)
        v = f.integral(mu2, cov2)
        b = f.sq_integral(mu2, cov2, want_r=True)
        assert not _same(a, b)
        assert _same(f.sq_integral(mu, cov, want_r=True), a)
        assert _same(f.sq_integral(mu2, cov2, want_r=True), b)
        assert f.integral(mu2, cov2) == v
    finally:
        f.close()


def test_noisy_gains_are_the_variance_after_append_at_the_mean(engine, oracle):
    """End to end on the device: after sq_integral_design with nugget = s^2, append the picks with
    targets equal to the posterior mean there; sq_integral's variance then equals zvar0 - sum gain
    within the variance tolerance."""
    n, d, s, A, scale, q, t = 130, 3, 0.1, 200, 1.0, 24, 10
    pc = _pieces(oracle, n, d, s, A, scale)
    mu, cov = _measure(d)
    piv, gain, zvar0 = _device(engine, n, d, s, A, scale, q, True)[:3]
    fit, xc = _fit(engine, n, d, s, A, scale)
    try:
        xp = np.asfortranarray(xc[:, piv[:t]])
        fit.append(xp, fit.predict(xp)[0])
        sq, var = fit.sq_integral(mu, cov)
    finally:
        fit.close()
    ld = _along(pc["sig"], pc["ld"]["u0"], pc["ld"]["zvar0"], piv, s * s)
    tg, tz = _tolerance(pc, piv, s * s, ld, "append")[:2]
    e1 = abs(float(zvar0 - np.sum(gain[:t]) - ld["zvar"][t]))
    e2 = abs(float(var - ld["zvar"][t]))
    e3 = abs(float(var - (zvar0 - np.sum(gain[:t]))))
    print("after %d picks: telescoped error / tol %.3g, appended error / tol %.3g, difference / tol "
          "%.3g" % (t, e1 / (tz + t * tg), e2 / tz, e3 / tz))
    assert e1 <= tz + t * tg and e2 <= tz
    assert e3 <= tz


def _outs(q, A):
    return dict(piv=np.full(q, 7, dtype=np.int64), gain=np.full(q, 7.0), zvar0=np.full(1, 7.0),
                ru=np.full(A, 7.0), rc=np.full(A, 7.0), s0=np.full(A, 7.0),
                rank=np.full(1, 7, dtype=np.int64))


def _raw(engine, fit, mu, cov, xc, A, q, nugget, tol, o):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def p(a, t=dp):
        return None if a is None else a.ctypes.data_as(t)

    return engine._lib.bq_gp_sqdesign(engine._ctx, fit._handle(), p(mu), p(cov), p(xc), A, q,
                                      nugget, tol, p(o["piv"], ip), p(o["gain"]), p(o["zvar0"]),
                                      p(o["ru"]), p(o["rc"]), p(o["s0"]), p(o["rank"], ip))


def _raw_integral(engine, fit, mu, cov, sq, var, r):
    dp = C.POINTER(C.c_double)

    def p(a):
        return None if a is None else a.ctypes.data_as(dp)

    return engine._lib.bq_gp_sqintegral(engine._ctx, fit._handle(), p(mu), p(cov), p(sq), p(var),
                                        p(r))


def test_argument_errors_write_nothing(engine):
    x, _, h, w, s, xc = _case(40, 2, 0.3, 10, 1.0)
    A, n = 10, 40
    mu, cov = _measure(2)
    fit = engine.gp_fit(x, _targets(x), h, w, s)
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
        m, v, r = np.full(1, 7.0), np.full(1, 7.0), np.full(n, 7.0)
        for bmu, bcov in ((bad_mu(np.nan), cov), (mu, bad_cov(np.inf)), (mu, not_pd), (None, cov),
                          (mu, None)):
            assert _raw_integral(engine, fit, bmu, bcov, m, v, r) != 0
            assert m[0] == 7 and v[0] == 7 and np.all(r == 7)
        assert _raw_integral(engine, fit, mu, cov, None, None, None) != 0
        assert _raw_integral(engine, fit, mu, cov, None, v, None) == 0 and v[0] != 7
        assert _raw_integral(engine, fit, mu, cov, m, None, None) == 0 and m[0] != 7
        assert _raw_integral(engine, fit, mu, cov, None, None, r) == 0 and np.all(r != 7)
        assert (m[0], v[0]) == fit.sq_integral(mu, cov)
        for bmu, bcov in ((bad_mu(np.nan), cov), (mu, not_pd)):
            with pytest.raises(ValueError):
                fit.sq_integral(bmu, bcov)
            with pytest.raises(ValueError):
                fit.sq_integral_design(xc, 2, bmu, bcov)
        with pytest.raises(ValueError):
            fit.sq_integral_design(xc, A + 1, mu, cov)
        with pytest.raises(ValueError):
            fit.sq_integral_design(np.zeros((3, 4)), 2, mu, cov)
        # A = 0: rank 0, the tails and zvar0, nothing else touched
        o = _outs(4, A)
        assert call(o, A=0, xc=None) == 0
        assert o["rank"][0] == 0 and np.all(o["piv"] == -1) and np.all(o["gain"] == 0.0)
        assert o["zvar0"][0] == v[0]
        assert np.all(o["ru"] == 7.0) and np.all(o["rc"] == 7.0) and np.all(o["s0"] == 7.0)
        # optional outputs may be missing
        want = fit.sq_integral_design(xc, 4, mu, cov, want_scores=True)
        o = _outs(4, A)
        o.update(ru=None, rc=None, s0=None)
        assert call(o) == 0
        assert o["rank"][0] == 4 and np.array_equal(o["piv"], want[0])
        assert np.array_equal(o["gain"], want[1]) and o["zvar0"][0] == want[2]
        # a single step over a single candidate
        one = fit.sq_integral_design(np.asfortranarray(xc[:, :1]), 1, mu, cov, nugget=s * s,
                                     want_scores=True)
        assert list(one[0]) == [0] and one[1][0] == one[5][0] > 0
        # stale targets: the handle's status rule, nothing written
        fit.set_y(_targets(x) * 1.5)
        o = _outs(4, A)
        assert call(o) != 0 and all(np.all(v == 7) for v in o.values())
        m[0] = 7.0
        assert _raw_integral(engine, fit, mu, cov, m, None, None) != 0 and m[0] == 7
        fit.refit(h, w, s)
        assert np.all(np.isfinite(fit.predict(xc)[1]))
    finally:
        fit.close()
