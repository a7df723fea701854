"""The designs that minimise the integrated posterior variance on the device (bq_gp_ivr,
engine.Fit.ivr_design) against explicit CPU references.

Points are test_gp_sample.py's ``_case(n, d, s, R + A, scale)``, the first R columns the reference
points and the last A the candidates, so that its ``_reference`` gives Sigma_ref (numpy.longdouble)
over the joint set; the weights are RandomState(7).uniform(0.5, 1.5, R), normalised.

The device is held to the recurrence of include/bqhip.h in long double on Sigma_ref along the
device's own pivots (``_along``): gain, ivar0, resid_r, resid_c and score0.  Each device pivot is
greedy within the tolerance -- its long-double score is within tol of the largest -- and
sum rho resid_r = ivar0 - sum gain.  The pivots equal those of the free long-double recurrence
after the test has asserted, on the reference alone, that every step's best score leads the second
by at least 1000 tolerances, that every gain is positive and that the smallest eligible
dc + nugget stays above 1.5e-3 k0.

The tolerance is measured, as in test_gp_pivchol.py: the float64 restatement
(test_gp_ivr_host.numpy_ivr) runs on the device's algebra -- the oracle's Gram, Cholesky,
triangular solve and K - V V^T -- along the device's pivots, and its largest error against the
long-double recurrence gives r relative to T = max diag K + max_i ||v_i||^2 (variances) or
T sum rho (gains, ivar0, scores); the device gets 100 max(r, 4 eps) times that scale."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gp_ivr_host import numpy_ivr
from test_gp_pivchol import _ld_solve_spd
from test_gp_sample import _case, _ld_gram, _reference
from test_gp_sample_host import kernel_scale

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0
LD = np.longdouble

# (n, d, s, R, A, w scale, q, noisy): one row block each; R off a 64 boundary and four candidate
# row blocks, with and without a nugget; three reference slices (R = 130, R = 192: Rp = 192 in
# slices of 64); six candidate row blocks and npad + q past 256 (n = 200: npad = 256); d = 1, where
# a candidate is taken twice; one candidate; one reference point
CASES = [
    (65, 3, 0.1, 64, 64, 1.0, 16, True),
    (130, 3, 0.1, 100, 200, 1.0, 24, True),
    (130, 3, 0.1, 100, 200, 1.0, 24, False),
    (130, 2, 0.05, 130, 70, 0.5, 32, True),
    (130, 2, 0.05, 130, 70, 0.5, 32, False),
    (200, 3, 0.1, 70, 330, 1.0, 40, True),
    (130, 3, 0.1, 192, 136, 1.0, 24, True),
    (65, 1, 0.1, 40, 64, 0.25, 12, True),
    (70, 2, 0.05, 63, 1, 0.5, 1, True),
    (70, 2, 0.05, 1, 63, 0.5, 9, False),
]


def _weights(R):
    rho = np.random.RandomState(7).uniform(0.5, 1.5, R)
    return rho / rho.sum()


def _nu(s, noisy):
    return s * s if noisy else 0.0


def _along(T0, SP, dc0, dr0, rho, piv, nu):
    """The recurrence along the pivots ``piv`` on T0 = Sigma(xc, xr), SP = Sigma(xc, xc[:, piv]) and
    the two diagonals (dr0 None: the candidates are the reference points), in T0's precision:
    {"scores": every step's score vector, -inf where not eligible; "gain"; "ivar": sum rho dr
    before every step and after the last; "den2": every step's smallest eligible dc + nu;
    "dr"; "dc"}."""
    dt = T0.dtype.type
    rho = rho.astype(T0.dtype)
    T, dc = T0.copy(), dc0.copy()
    dr = dc if dr0 is None else dr0.copy()
    A, q = T.shape[0], len(piv)
    Cf = np.zeros((A, q), dtype=T0.dtype)
    taken = np.zeros(A, dtype=bool)
    out = {"scores": [], "gain": [], "ivar": [rho @ dr], "den2": []}
    for t, p in enumerate(piv):
        den2 = dc + dt(nu)
        ok = (den2 > 0) & ~taken if nu == 0 else den2 > 0
        sc = np.full(A, -np.inf, dtype=T0.dtype)
        sc[ok] = ((T * T) @ rho)[ok] / den2[ok]
        out["scores"].append(sc)
        out["gain"].append(sc[p])
        out["den2"].append(den2[ok].min())
        den = np.sqrt(den2[p])
        c = (SP[:, t] - Cf[:, :t] @ Cf[p, :t]) / den
        if nu == 0:
            c[taken] = 0
            c[p] = den
            taken[p] = True
        u = T[p] / den
        T -= np.outer(c, u)
        dc -= c * c
        if dr0 is not None:
            dr -= u * u
        if nu == 0:
            dc[taken] = 0
        Cf[:, t] = c
        out["ivar"].append(rho @ dr)
    out["gain"] = np.array(out["gain"], dtype=T0.dtype)
    out["dr"], out["dc"] = dr, dc
    return out


def _pieces(S, R, piv):
    """_along's inputs out of a covariance over [R reference points | candidates] in long double
    (R == 0: the candidates are the reference points)."""
    S = S.astype(LD)
    d = np.diag(S).copy()
    if R == 0:
        return S.copy(), S[:, piv], d, None
    return S[R:, :R].copy(), S[R:, R + np.asarray(piv, dtype=np.int64)], d[R:], d[:R]


def _errors(dev, ld, rho):
    """(the largest error of gain, ivar0 and score0; that of resid_r and resid_c) of a result
    (piv, gain, ivar0, resid_r, resid_c, score0) against _along's."""
    piv, gain, ivar0, rr, rc, s0 = dev
    s0_ld = np.where(np.isfinite(ld["scores"][0]), ld["scores"][0], 0) if len(piv) else s0
    eg = max(float(np.max(np.abs(gain - ld["gain"]))) if len(piv) else 0.0,
             float(abs(ivar0 - ld["ivar"][0])), float(np.max(np.abs(s0 - s0_ld))))
    ev = max(float(np.max(np.abs(rr - ld["dr"]))), float(np.max(np.abs(rc - ld["dc"]))))
    return eg, ev


def _tolerance(ref, R, rho, piv, nu, ld, label):
    """(tol for gains, ivar0 and scores; tol for variances): 100 max(r, 4 eps) (T sum rho; T) with
    r from the float64 restatement on the device's algebra along the device's pivots."""
    sig, T, k0, cpu = ref
    out = numpy_ivr(np.array(cpu), R, rho, k0, len(piv), nu, 0.0, pivots=piv)
    r = float(np.max(np.abs(cpu - sig))) / T
    if out[6] == len(piv):
        eg, ev = _errors((piv,) + out[1:6], ld, rho)
        r = max(r, eg / (T * rho.sum()), ev / T)
    print("%s: r %.3g" % (label, r))
    m = MARGIN * max(r, 4 * EPS)
    return m * T * rho.sum(), m * T


@functools.lru_cache(maxsize=None)
def _device(engine, n, d, s, R, A, scale, q, noisy, same=False):
    x, y, h, w, s, xo = _case(n, d, s, R + A, scale)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        if same:
            out = fit.ivr_design(xo, q, rho=_weights(A), nugget=_nu(s, noisy), want_scores=True)
        else:
            out = fit.ivr_design(np.asfortranarray(xo[:, R:]), q, xr=np.asfortranarray(xo[:, :R]),
                                 rho=_weights(R), nugget=_nu(s, noisy), want_scores=True)
    finally:
        fit.close()
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _check_against_reference(dev, ref, R, rho, nu, q, label):
    """A result against the long-double recurrence along its own pivots: the values, greedy within
    the tolerance, the telescoping sum.  Returns the tolerances."""
    sig, T, k0, _ = ref
    piv, gain, ivar0, rr, rc, s0 = dev
    ld = _along(*_pieces(sig, R, piv), rho, piv, nu)
    tg, tv = _tolerance(ref, R, rho, piv, nu, ld, label)
    eg, ev = _errors(dev, ld, rho)
    short = max(float(np.max(sc) - sc[p]) for sc, p in zip(ld["scores"], piv))
    # every term of ivar0 - sum gain - rho . resid_r is within tg of its exact value
    tele = abs(float(rho @ rr) - (ivar0 - float(np.sum(gain))))
    print("%s: value error / tol %.3g, variance error / tol %.3g, greedy shortfall / tol %.3g, "
          "telescoping / tol %.3g, smallest gain / ivar0 %.3g"
          % (label, eg / tg, ev / tv, short / tg, tele / tg, float(np.min(gain)) / ivar0))
    assert eg <= tg and ev <= tv and short <= tg
    assert tele <= (q + 2) * tg
    return tg, tv


@pytest.mark.parametrize("n,d,s,R,A,scale,q,noisy", CASES)
def test_design_holds_its_contract(engine, oracle, n, d, s, R, A, scale, q, noisy):
    ref = _reference(oracle, n, d, s, R + A, scale)
    nu, rho = _nu(s, noisy), _weights(R)
    dev = _device(engine, n, d, s, R, A, scale, q, noisy)
    piv, gain, ivar0, rr, rc, s0 = dev
    label = "n=%d d=%d R=%d A=%d q=%d nu=%g" % (n, d, R, A, q, nu)
    assert piv.shape == (q,) and piv.dtype == np.int64 and gain.shape == (q,)  # full rank
    assert rr.shape == (R,) and rc.shape == (A,) and s0.shape == (A,) and isinstance(ivar0, float)
    assert np.all((piv >= 0) & (piv < A)) and np.all(gain > 0)
    assert np.all(np.isfinite(rr)) and np.all(np.isfinite(rc)) and np.all(np.isfinite(s0))
    assert s0[piv[0]] == gain[0] == s0.max() and piv[0] == int(np.argmax(s0))
    _check_against_reference(dev, ref, R, rho, nu, q, label)
    if nu == 0.0:
        assert len(set(piv.tolist())) == q and np.all(rc[piv] == 0.0)
    else:
        assert np.all(rc > 0) and np.all(rr > 0)
    if d == 1:
        assert len(set(piv.tolist())) < q  # a candidate taken twice


@pytest.mark.parametrize("n,d,s,R,A,scale,q,noisy", CASES)
def test_pivots_are_the_reference_s(engine, oracle, n, d, s, R, A, scale, q, noisy):
    ref = _reference(oracle, n, d, s, R + A, scale)
    sig, T, k0, _ = ref
    nu, rho = _nu(s, noisy), _weights(R)
    want, wgain, wivar0, _, _, _, rank = numpy_ivr(sig.astype(LD), R, rho, LD(k0), q, nu, 0.0)
    assert rank == q and np.all(wgain > 0)
    # the conditions that make the comparison fair, on the reference alone
    ld = _along(*_pieces(sig, R, want), rho, want, nu)
    leads = []
    for sc, p in zip(ld["scores"], want):
        rest = np.delete(sc, p)
        rest = rest[np.isfinite(rest)]
        leads.append(float(sc[p] - np.max(rest)) if rest.size else np.inf)
    tg, _ = _tolerance(ref, R, rho, want, nu, ld, "n=%d R=%d A=%d q=%d" % (n, R, A, q))
    den2 = float(min(ld["den2"]))
    print("smallest lead %.3g ivar0 = %.3g tol, smallest dc + nu %.3g k0, smallest gain %.3g ivar0"
          % (min(leads) / float(wivar0), min(leads) / tg, den2 / k0,
             float(np.min(wgain) / wivar0)))
    assert min(leads) >= 1000 * tg
    assert den2 >= 1.5e-3 * k0
    piv, gain = _device(engine, n, d, s, R, A, scale, q, noisy)[:2]
    assert np.array_equal(piv, want)
    assert float(np.max(np.abs(gain - wgain.astype(np.float64)))) <= tg


def test_prefix_property_and_same_bits(engine):
    n, d, s, R, A, scale, q = 130, 3, 0.1, 100, 200, 1.0, 24
    x, y, h, w, s, xo = _case(n, d, s, R + A, scale)
    xr, xc, rho = np.asfortranarray(xo[:, :R]), np.asfortranarray(xo[:, R:]), _weights(R)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        for nu in (0.0, s * s):
            for kw in (dict(xr=xr, rho=rho), dict(rho=_weights(A))):
                full = fit.ivr_design(xc, q, nugget=nu, want_scores=True, **kw)
                again = fit.ivr_design(xc, q, nugget=nu, want_scores=True, **kw)
                assert all(np.array_equal(a, b) for a, b in zip(full, again))
                for j in (1, 17, q):
                    part = fit.ivr_design(xc, j, nugget=nu, want_scores=True, **kw)
                    assert np.array_equal(part[0], full[0][:j])
                    assert np.array_equal(part[1], full[1][:j])
                    assert part[2] == full[2] and np.array_equal(part[5], full[5])
                # without the scores: the same
                bare = fit.ivr_design(xc, q, nugget=nu, **kw)
                assert len(bare) == 5 and all(np.array_equal(a, b) for a, b in zip(bare, full))
        # the sweep under it is bq_gp_predict's: a stop level above every gain leaves its variances
        var_r, var_c = fit.predict(xr)[1], fit.predict(xc)[1]
        p0, g0, ivar0, rr, rc = fit.ivr_design(xc, 1, xr=xr, rho=rho, tol=10.0)
        assert p0.shape == (0,) and g0.shape == (0,)
        assert np.array_equal(rr, var_r) and np.array_equal(rc, var_c)
        assert abs(ivar0 - rho @ var_r) <= 4 * EPS * ivar0
        # uniform weights by default
        a = fit.ivr_design(xc, 3, xr=xr)
        b = fit.ivr_design(xc, 3, xr=xr, rho=np.full(R, 1.0 / R))
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    finally:
        fit.close()


@pytest.mark.parametrize("noisy", [True, False])
def test_candidates_as_their_own_reference(engine, oracle, noisy):
    """xr = None against xr = xc: one sweep over A points against one over two copies of them.
    Both are held to the long-double recurrence on Sigma_ref over the A points, and -- the
    reference's leads being 1000 tolerances -- take the same pivots."""
    n, d, s, A, scale, q = 130, 3, 0.1, 200, 1.0, 24
    ref = _reference(oracle, n, d, s, A, scale)
    sig, T, k0, _ = ref
    x, y, h, w, s, xo = _case(n, d, s, A, scale)
    nu, rho = _nu(s, noisy), _weights(A)
    one = _device(engine, n, d, s, 0, A, scale, q, noisy, True)
    assert one[3] is one[4]
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        two = fit.ivr_design(xo, q, xr=xo, rho=rho, nugget=nu, want_scores=True)
    finally:
        fit.close()
    label = "A=%d q=%d nu=%g" % (A, q, nu)
    tg, tv = _check_against_reference(one, ref, 0, rho, nu, q, label + ", xr=None")
    ld = _along(*_pieces(sig, 0, two[0]), rho, two[0], nu)
    eg, ev = _errors(two, ld, rho)
    print("%s, xr=xc: value error / tol %.3g, variance error / tol %.3g" % (label, eg / tg, ev / tv))
    assert eg <= tg and ev <= tv
    want = numpy_ivr(sig.astype(LD), 0, rho, LD(k0), q, nu, 0.0)[0]
    free = _along(*_pieces(sig, 0, want), rho, want, nu)
    lead = min(float(sc[p] - np.max(np.delete(sc, p))) for sc, p in zip(free["scores"], want))
    assert lead >= 1000 * tg
    assert np.array_equal(one[0], want) and np.array_equal(two[0], want)
    assert float(np.max(np.abs(one[1] - two[1]))) <= 2 * tg
    assert float(np.max(np.abs(one[4] - two[4]))) <= 2 * tv
    assert float(np.max(np.abs(two[3] - two[4]))) <= 2 * tv


def test_noisy_resid_is_the_variance_after_append(engine, oracle):
    """With nugget = s^2 the variances left are those of a fit that has appended the chosen
    candidates with arbitrary targets.  Both are held to the closed form on Sigma_ref in long
    double; the tolerance is measured on the float64 closed form over the device's algebra.  The
    pivoted Cholesky's variances: over the chosen points alone it takes each of them once -- the
    same pivots as a set, and with a nugget the variances left do not depend on the order -- so
    its resid is resid_c at the pivots."""
    n, d, s, R, A, scale, q = 130, 3, 0.1, 100, 200, 1.0, 24
    ref = _reference(oracle, n, d, s, R + A, scale)
    sig, T, k0, cpu = ref
    x, y, h, w, s, xo = _case(n, d, s, R + A, scale)
    xr, xc = np.asfortranarray(xo[:, :R]), np.asfortranarray(xo[:, R:])
    nu = s * s
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        piv, _, _, rr, rc = fit.ivr_design(xc, q, xr=xr, rho=_weights(R), nugget=nu)
        chosen = np.asfortranarray(xc[:, piv])
        piv2, _, resid2, _ = fit.pivoted_cholesky(chosen, q, nugget=nu, want_factor=False)
        fit.append(chosen, np.random.RandomState(5).randn(q))
        var = fit.predict(xo)[1]
    finally:
        fit.close()
    assert len(set(piv.tolist())) == q and sorted(piv2.tolist()) == list(range(q))
    P = R + piv
    S = sig.astype(LD)
    Am = S[np.ix_(P, P)] + LD(nu) * np.eye(q, dtype=LD)
    closed = np.diag(S) - np.sum(S[:, P] * _ld_solve_spd(Am, S[P, :]).T, axis=1)
    cl64 = np.diag(cpu) - np.sum(cpu[:, P] * np.linalg.solve(
        cpu[np.ix_(P, P)] + nu * np.eye(q), cpu[P, :]).T, axis=1)
    r = max(float(np.max(np.abs(cl64 - closed))), float(np.max(np.abs(cpu - sig)))) / T
    tol = MARGIN * max(r, 4 * EPS) * T
    resid = np.concatenate([rr, rc])
    e1, e2 = float(np.max(np.abs(resid - closed))), float(np.max(np.abs(var - closed)))
    print("r %.3g; resid error / tol %.3g, appended variance error / tol %.3g"
          % (r, e1 / tol, e2 / tol))
    assert e1 <= tol and e2 <= tol
    assert float(np.max(np.abs(resid - var))) <= 2 * tol
    assert float(np.max(np.abs(rc[piv] - resid2))) <= 2 * tol


def _raw(engine, fit, xr, R, rho, xc, A, q, nugget, tol, piv, gain, ivar0, rr, rc, s0, rank):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def p(a, t=dp):
        return None if a is None else a.ctypes.data_as(t)

    return engine._lib.bq_gp_ivr(engine._ctx, fit._handle(), p(xr), R, p(rho), p(xc), A, q, nugget,
                                 tol, p(piv, ip), p(gain), p(ivar0), p(rr), p(rc), p(s0),
                                 p(rank, ip))


def test_argument_errors_write_nothing(engine):
    x, y, h, w, s, xo = _case(40, 2, 0.3, 16, 1.0)
    R, A = 6, 10
    xr, xc, rho = np.asfortranarray(xo[:, :R]), np.asfortranarray(xo[:, R:]), _weights(R)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        def outs():
            return dict(piv=np.full(4, 7, dtype=np.int64), gain=np.full(4, 7.0),
                        ivar0=np.full(1, 7.0), rr=np.full(R, 7.0), rc=np.full(A, 7.0),
                        s0=np.full(A, 7.0), rank=np.full(1, 7, dtype=np.int64))

        def call(o, **kw):
            a = dict(xr=xr, R=R, rho=rho, xc=xc, A=A, q=4, nugget=0.0, tol=0.0)
            a.update(kw)
            return _raw(engine, fit, a["xr"], a["R"], a["rho"], a["xc"], a["A"], a["q"],
                        a["nugget"], a["tol"], o["piv"], o["gain"], o["ivar0"], o["rr"], o["rc"],
                        o["s0"], o["rank"])

        def bad_rho(v):
            b = rho.copy()
            b[2] = v
            return b

        bad = [dict(A=-1), dict(R=-1), dict(q=0), dict(q=-3), dict(q=A + 1), dict(nugget=-1e-3),
               dict(nugget=np.nan), dict(nugget=np.inf), dict(tol=-1e-3), dict(tol=np.nan),
               dict(tol=np.inf), dict(rho=bad_rho(-1e-3)), dict(rho=bad_rho(np.nan)),
               dict(rho=bad_rho(np.inf)), dict(rho=None), dict(xc=None), dict(xr=None),
               dict(R=0), dict(R=2 ** 20 - A + 1, q=1), dict(A=2 ** 20 + 1, q=1),
               dict(R=2 ** 14 + 1, A=2 ** 14, q=1),  # Rp Ap = (2^14 + 64) 2^14 > 2^28 entries of T
               dict(q=2 ** 16 + 1, A=2 ** 17, R=64)]
        for kw in bad:
            o = outs()
            assert call(o, **kw) != 0, kw
            assert all(np.all(v == 7) for v in o.values()), kw
        for drop in ("piv", "gain", "ivar0", "rank"):
            o = outs()
            keep = dict(o)
            o[drop] = None
            assert call(o) != 0, drop
            assert all(np.all(v == 7) for v in keep.values()), drop
        with pytest.raises(ValueError):
            fit.ivr_design(xc, 0, xr=xr)
        with pytest.raises(ValueError):
            fit.ivr_design(np.zeros((3, 4)), 2)
        with pytest.raises(ValueError):
            fit.ivr_design(xc, 2, xr=np.zeros((3, 4)))
        with pytest.raises(ValueError):
            fit.ivr_design(xc, 2, xr=xr, rho=np.full(R + 1, 0.1))
        # A = 0: rank 0, the tails and ivar0 = 0, nothing else touched
        o = outs()
        assert call(o, A=0, xc=None) == 0
        assert o["rank"][0] == 0 and np.all(o["piv"] == -1) and np.all(o["gain"] == 0.0)
        assert o["ivar0"][0] == 0.0
        assert np.all(o["rr"] == 7.0) and np.all(o["rc"] == 7.0) and np.all(o["s0"] == 7.0)
        o = outs()
        assert call(o, A=0, xc=None, xr=None, R=0, rho=None) == 0 and o["rank"][0] == 0
        # optional outputs may be missing
        want = fit.ivr_design(xc, 4, xr=xr, rho=rho, want_scores=True)
        o = outs()
        o.update(rr=None, rc=None, s0=None)
        assert call(o) == 0
        assert o["rank"][0] == 4 and np.array_equal(o["piv"], want[0])
        assert np.array_equal(o["gain"], want[1]) and o["ivar0"][0] == want[2]
        # all of them, and the tails of a run that a stop level ends: between two gains
        level = float(np.sqrt(want[1][1] * want[1][2])) / (kernel_scale(h, w) * rho.sum())
        o = outs()
        assert call(o, tol=level) == 0
        assert o["rank"][0] == 2 and np.array_equal(o["piv"][:2], want[0][:2])
        assert np.all(o["piv"][2:] == -1) and np.all(o["gain"][2:] == 0.0)
        assert np.array_equal(o["gain"][:2], want[1][:2]) and np.array_equal(o["s0"], want[5])
        two = fit.ivr_design(xc, 2, xr=xr, rho=rho)
        assert np.array_equal(o["rr"], two[3]) and np.array_equal(o["rc"], two[4])
        # xr = NULL: resid_r receives the candidates' variances
        o = outs()
        o["rr"] = np.full(A, 7.0)
        assert call(o, xr=None, R=0, rho=_weights(A)) == 0
        assert o["rank"][0] == 4 and np.array_equal(o["rr"], o["rc"]) and np.all(o["rc"][o["piv"]] == 0)
        # all-zero weights: nothing to gain
        o = outs()
        assert call(o, rho=np.zeros(R)) == 0
        assert o["rank"][0] == 0 and o["ivar0"][0] == 0.0 and np.all(o["s0"] == 0.0)
        assert np.array_equal(o["rc"], fit.predict(xc)[1])
        # the fit is not disturbed
        assert np.all(np.isfinite(fit.predict(xo)[1]))
    finally:
        fit.close()


def _big_pieces(x, h, w, s, xr, xc, P, oracle=None):
    """(T0, SP, dc0, dr0, T): _along's inputs from the definition in long double, or -- with the
    oracle -- by the device's algebra in float64 (Cholesky, triangular solve, K - V V^T).  Only
    the columns of Sigma(xc, xc) at the pivots are formed."""
    xcP = np.asfortranarray(xc[:, P])
    if oracle is None:
        n = x.shape[1]
        Am = _ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD)
        Kcx, Krx = _ld_gram(xc, x, h, w), _ld_gram(xr, x, h, w)
        Zc, Zr = _ld_solve_spd(Am, Kcx.T), _ld_solve_spd(Am, Krx.T)
        k0 = _ld_gram(xc[:, :1], xc[:, :1], h, w)[0, 0]
        return (_ld_gram(xc, xr, h, w) - Kcx @ Zr, _ld_gram(xc, xcP, h, w) - Kcx @ Zc[:, P],
                k0 - np.sum(Kcx * Zc.T, axis=1), k0 - np.sum(Krx * Zr.T, axis=1), None)
    from scipy.linalg import solve_triangular
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    Vc = solve_triangular(Lc, np.ascontiguousarray(oracle.gram_cross(x, xc, h, w)), lower=True).T
    Vr = solve_triangular(Lc, np.ascontiguousarray(oracle.gram_cross(x, xr, h, w)), lower=True).T
    k0 = float(np.asarray(oracle.gram(xc[:, :1], h, w, 0.0))[0, 0])
    vc, vr = np.sum(Vc * Vc, axis=1), np.sum(Vr * Vr, axis=1)
    return (np.asarray(oracle.gram_cross(xc, xr, h, w)) - Vc @ Vr.T,
            np.asarray(oracle.gram_cross(xc, xcP, h, w)) - Vc @ Vc[P].T, k0 - vc, k0 - vr,
            k0 + float(max(vc.max(), vr.max())))


@pytest.mark.parametrize("R,A,noisy", [(64, 16384, False), (64, 16384, True), (16500, 64, True)])
def test_larger_launch_shapes(engine, oracle, R, A, noisy):
    """The sizes at which the launches take another shape: 256-candidate workgroups of the pass
    over T and of the product from Ap = 16384 on, with more candidates than the picking workgroup
    has threads' worth of one block; and 258 reference slices of 64 columns over one candidate
    block, 65 workgroups of reference points in the column kernel.  Sigma(xc, xc) does not fit a
    test at the first: the recurrence needs T, the columns of Sigma(xc, xc) at the pivots and the
    diagonals, all from the definition in long double, the tolerance measured on the same pieces
    by the device's algebra in float64 along the device's pivots.  Held to the values, the
    telescoping sum and greedy-within-tolerance, not to exact pivots."""
    n, d, s, scale, q = 40, 2, 0.3, 1.0, 6
    x, y, h, w, s, xo = _case(n, d, s, R + A, scale)
    xr, xc, rho = np.asfortranarray(xo[:, :R]), np.asfortranarray(xo[:, R:]), _weights(R)
    nu = _nu(s, noisy)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        dev = fit.ivr_design(xc, q, xr=xr, rho=rho, nugget=nu, want_scores=True)
        half = fit.ivr_design(xc, q // 2, xr=xr, rho=rho, nugget=nu)
    finally:
        fit.close()
    piv, gain, ivar0, rr, rc, s0 = dev
    assert piv.shape == (q,) and rr.shape == (R,) and rc.shape == (A,) and s0.shape == (A,)
    assert np.array_equal(half[0], piv[:q // 2]) and np.array_equal(half[1], gain[:q // 2])
    T0, SP, dc0, dr0, _ = _big_pieces(x, h, w, s, xr, xc, piv)
    ld = _along(T0, SP, dc0, dr0, rho, piv, nu)
    p64 = _big_pieces(x, h, w, s, xr, xc, piv, oracle)
    T = p64[4]
    f64 = _along(*p64[:4], rho, piv, nu)
    s64 = np.where(np.isfinite(f64["scores"][0]), f64["scores"][0], 0)
    eg, ev = _errors((piv, f64["gain"], f64["ivar"][0], f64["dr"], f64["dc"], s64), ld, rho)
    r = max(eg / (T * rho.sum()), ev / T, float(np.max(np.abs(p64[0] - T0))) / T,
            float(np.max(np.abs(p64[1] - SP))) / T)
    m = MARGIN * max(r, 4 * EPS)
    tg, tv = m * T * rho.sum(), m * T
    eg, ev = _errors(dev, ld, rho)
    short = max(float(np.max(sc) - sc[p]) for sc, p in zip(ld["scores"], piv))
    tele = abs(float(rho @ rr) - (ivar0 - float(np.sum(gain))))
    print("R=%d A=%d nu=%g: r %.3g; value error / tol %.3g, variance error / tol %.3g, greedy "
          "shortfall / tol %.3g, telescoping / tol %.3g"
          % (R, A, nu, r, eg / tg, ev / tv, short / tg, tele / tg))
    assert eg <= tg and ev <= tv and short <= tg and tele <= (q + 2) * tg
    if nu == 0.0:
        assert len(set(piv.tolist())) == q and np.all(rc[piv] == 0.0)
