"""The pivoted partial Cholesky of a posterior on the device (bq_gp_pivchol,
engine.Fit.pivoted_cholesky) against explicit CPU references.

The factor is held to its contract, not to another factor.  With P the device's pivots,
Sigma_ref from mpmath at 50 digits (n, M <= 65) or numpy.longdouble (test_gp_sample.py's
helpers) and L the lower triangle of C[P, :] whose diagonal is sqrt(gain + nugget):
    C L^T = Sigma_ref[:, P],   L L^T = Sigma_ref[P, P] + nugget I,
    resid = diag Sigma_ref - rowsum(C^2)
          = diag(Sigma_ref - Sigma_ref[:, P] (Sigma_ref[P, P] + nugget I)^-1 Sigma_ref[P, :]),
    gain_j = C[p_j, j] sqrt(gain_j + nugget).
With nugget = 0, L is C[P, :] itself and these are C C[P, :]^T = Sigma_ref[:, P] and
gain_j = C[p_j, j]^2, together with the exact zeros.  (With a nugget C[P, :] = L - nugget L^-T:
its diagonal is gain / sqrt(gain + nugget), so the identities are stated through L; that resid
is the variance after noisy observations needs exactly this C.)

The tolerance is measured, as in test_gp_sample.py and test_predict_grad.py: the float64 numpy
restatement (test_gp_pivchol_host.numpy_pivchol) runs on the device's algebra -- Cholesky,
triangular solve, Koo - V V^T, then the recurrence along the device's own pivots -- and the
largest error of the same identities gives r relative to T = max diag K(xo, xo) +
max_i ||v_i||^2; the device gets 100 max(r, 4 eps) T.

Pivots: on the d >= 2 cases the device's pivots equal those of the recurrence in long double on
Sigma_ref, after the test has asserted on the reference alone that the best candidate leads the
second best by at least 1000 tolerances at every step.  On every case each device pivot is
greedy within the tolerance: d^(j), recomputed in long double along the device's earlier pivots,
has d^(j)[p_j] >= max d^(j) - tol.

BQ_GUARD and bq_plan_check_guards cover the buffers of a plan, not those of a fit, so there is
no guard-band test here."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gp_pivchol_host import numpy_pivchol
from test_gp_sample import _case, _reference

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MARGIN = 100.0
LD = np.longdouble

# (n, d, s, M, w scale, q, noisy): Mp = 128 with q = M; two and four row blocks; a nugget; npad + q
# across a 64-column boundary of the slices (n = 200: npad = 256, q = 64); one point; M below a
# row block; d = 1 with gaps down to 1e-7 k0
CASES = [
    (65, 3, 0.1, 65, 1.0, 65, False),
    (130, 3, 0.1, 200, 1.0, 48, False),
    (130, 3, 0.1, 200, 1.0, 48, True),
    (130, 2, 0.05, 130, 0.5, 65, False),
    (200, 3, 0.1, 320, 1.0, 64, False),
    (65, 1, 0.1, 64, 0.25, 32, False),
    (70, 2, 0.05, 1, 0.5, 1, False),
    (70, 2, 0.05, 63, 0.5, 17, False),
]
EXACT_PIVOT_CASES = [c for c in CASES[:5]]


def _ld_solve_spd(A, B):
    """A^-1 B in long double: an unblocked Cholesky and two substitutions."""
    n = A.shape[0]
    Lf = np.zeros((n, n), dtype=LD)
    for j in range(n):
        Lf[j, j] = np.sqrt(A[j, j] - Lf[j, :j] @ Lf[j, :j])
        Lf[j + 1:, j] = (A[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    X = np.array(B, dtype=LD)
    for j in range(n):
        X[j] = (X[j] - Lf[j, :j] @ X[:j]) / Lf[j, j]
    for j in range(n - 1, -1, -1):
        X[j] = (X[j] - Lf[j + 1:, j] @ X[j + 1:]) / Lf[j, j]
    return X


def _ld_trace(sig, piv, nu):
    """d^(j) before every step j, and d^(len(piv)), of the recurrence in long double on Sigma_ref
    along the given pivots (no zeroing: exact arithmetic needs none)."""
    S = sig.astype(LD)
    d = np.diag(S).copy()
    Cl = np.zeros((S.shape[0], len(piv)), dtype=LD)
    trace = []
    for j, p in enumerate(piv):
        trace.append(d.copy())
        c = (S[:, p] - Cl[:, :j] @ Cl[p, :j]) / np.sqrt(d[p] + LD(nu))
        Cl[:, j] = c
        d = d - c * c
    trace.append(d)
    return trace


def _identity_errors(Cf, resid, gain, P, sig, nu):
    """The largest absolute error of each identity of the module docstring, in long double."""
    S = sig.astype(LD)
    r = len(P)
    Cl, g = Cf.astype(LD), gain.astype(LD)
    Lf = np.tril(Cl[P], -1) + np.diag(np.sqrt(g + LD(nu)))
    A = S[np.ix_(P, P)] + LD(nu) * np.eye(r, dtype=LD)
    closed = np.diag(S) - np.sum(S[:, P] * _ld_solve_spd(A, S[P, :]).T, axis=1)
    return {
        "C L^T": float(np.max(np.abs(Cl @ Lf.T - S[:, P]))),
        "L L^T": float(np.max(np.abs(Lf @ Lf.T - A))),
        "resid, rowsum": float(np.max(np.abs(resid - (np.diag(S) - np.sum(Cl * Cl, axis=1))))),
        "resid, closed": float(np.max(np.abs(resid - closed))),
        "gain": float(np.max(np.abs(np.diag(Cl[P]) * np.sqrt(g + LD(nu)) - g))),
    }


def _tolerance(ref, P, nu, label):
    """100 max(r, 4 eps) T with r from the float64 restatement on the device's algebra along the
    device's pivots."""
    sig, T, k0, cpu = ref
    piv, Cc, resid, gain, rank = numpy_pivchol(np.array(cpu), k0, len(P), nu, 0.0, pivots=P)
    r = float(np.max(np.abs(cpu - sig))) / T
    if rank == len(P):
        errs = _identity_errors(Cc, resid, gain, P, sig, nu)
        r = max(r, max(errs.values()) / T)
    print("%s: r %.3g" % (label, r))
    return MARGIN * max(r, 4 * EPS) * T


@functools.lru_cache(maxsize=None)
def _device(engine, n, d, s, M, scale, q, noisy, tol=0.0, dup=False):
    x, y, h, w, s, xo = _case(n, d, s, M, scale, 0, dup)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        out = fit.pivoted_cholesky(xo, q, nugget=s * s if noisy else 0.0, tol=tol)
    finally:
        fit.close()
    for a in out:
        a.setflags(write=False)
    return out


def _nu(s, noisy):
    return s * s if noisy else 0.0


@pytest.mark.parametrize("n,d,s,M,scale,q,noisy", CASES)
def test_factor_holds_its_contract(engine, oracle, n, d, s, M, scale, q, noisy):
    ref = _reference(oracle, n, d, s, M, scale)
    sig, T, k0, _ = ref
    nu = _nu(s, noisy)
    piv, Cf, resid, gain = _device(engine, n, d, s, M, scale, q, noisy)
    label = "n=%d d=%d M=%d q=%d nu=%g" % (n, d, M, q, nu)
    assert piv.shape == (q,) and piv.dtype == np.int64 and gain.shape == (q,)  # full rank
    assert Cf.shape == (M, q) and Cf.flags.f_contiguous and resid.shape == (M,)
    assert np.all((piv >= 0) & (piv < M)) and np.all(gain > 0)
    assert np.all(np.isfinite(Cf)) and np.all(np.isfinite(resid))
    tol = _tolerance(ref, piv, nu, label)
    errs = _identity_errors(Cf, resid, gain, piv, sig, nu)
    for what, err in sorted(errs.items()):
        print("%s: %s error / tol %.3g" % (label, what, err / tol))
    assert all(err <= tol for err in errs.values()), (label, errs, tol)
    # greedy within the tolerance, step by step
    trace = _ld_trace(sig, piv, nu)
    short = max(float(np.max(t) - t[p]) for t, p in zip(trace, piv))
    print("%s: greedy shortfall / tol %.3g, smallest gain / k0 %.3g"
          % (label, short / tol, float(np.min(gain)) / k0))
    assert short <= tol
    assert float(np.max(np.abs(gain - np.array([t[p] for t, p in zip(trace, piv)])))) <= tol
    if nu == 0.0:
        assert len(set(piv.tolist())) == q
        assert np.all(Cf[piv][np.triu_indices(q, 1)] == 0.0)
        assert np.all(np.abs(np.diag(Cf[piv]) - np.sqrt(gain)) <= EPS * np.sqrt(gain))  # 1 ulp
        assert np.all(resid[piv] == 0.0)
    else:
        assert np.all(resid > 0)


@pytest.mark.parametrize("n,d,s,M,scale,q,noisy", EXACT_PIVOT_CASES)
def test_pivots_are_the_reference_s(engine, oracle, n, d, s, M, scale, q, noisy):
    ref = _reference(oracle, n, d, s, M, scale)
    sig, T, k0, _ = ref
    nu = _nu(s, noisy)
    piv, _, _, gain = _device(engine, n, d, s, M, scale, q, noisy)
    want, _, _, wgain, rank = numpy_pivchol(sig.astype(LD), LD(k0), q, nu, 0.0)
    assert rank == q
    # the condition that makes the comparison fair, on the reference alone
    trace = _ld_trace(sig, want, nu)
    gaps = []
    for t, p in zip(trace, want):
        rest = np.delete(t, p)
        gaps.append(float(t[p] - np.max(rest)) if rest.size else np.inf)
    tol = _tolerance(ref, want, nu, "n=%d M=%d q=%d" % (n, M, q))
    print("smallest gain %.3g k0, smallest gap %.3g k0 = %.3g tol"
          % (float(np.min(wgain)) / k0, min(gaps) / k0, min(gaps) / tol))
    assert min(gaps) >= 1000 * tol
    assert np.array_equal(piv, want)
    assert float(np.max(np.abs(gain - wgain.astype(np.float64)))) <= tol


def test_prefix_property_and_same_bits(engine):
    n, d, s, M, scale = 130, 3, 0.1, 200, 1.0
    x, y, h, w, s, xo = _case(n, d, s, M, scale)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        for nu in (0.0, s * s):
            full = fit.pivoted_cholesky(xo, 48, nugget=nu)
            again = fit.pivoted_cholesky(xo, 48, nugget=nu)
            assert all(np.array_equal(a, b) for a, b in zip(full, again))
            for j in (1, 17, 48):
                piv, Cf, resid, gain = fit.pivoted_cholesky(xo, j, nugget=nu)
                assert np.array_equal(piv, full[0][:j]) and np.array_equal(gain, full[3][:j])
                assert np.array_equal(Cf, full[1][:, :j])
            # without the factor: the same pivots and variances
            piv, none, resid, gain = fit.pivoted_cholesky(xo, 48, nugget=nu, want_factor=False)
            assert none is None and np.array_equal(piv, full[0])
            assert np.array_equal(resid, full[2]) and np.array_equal(gain, full[3])
        # the sweep under it is bq_gp_predict's: d^(0) is its variance
        var = fit.predict(xo)[1]
        p0, _, r0, g0 = fit.pivoted_cholesky(xo, 1, tol=10.0)
        assert p0.shape == (0,) and np.array_equal(r0, var)
        assert fit.pivoted_cholesky(xo, 1)[3][0] == var.max()
    finally:
        fit.close()


def _raw(engine, fit, xo, M, q, nugget, tol, piv, Cf, resid, gain, rank):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)

    def p(a, t=dp):
        return None if a is None else a.ctypes.data_as(t)

    return engine._lib.bq_gp_pivchol(engine._ctx, fit._handle(), p(xo), M, q, nugget, tol,
                                     p(piv, ip), p(Cf), p(resid), p(gain), p(rank, ip))


def test_stop_rule_and_tails(engine, oracle):
    """A stop level at the geometric mean of two of the reference's gains ends the factorisation
    between them; the tails are -1 and zeros.  The duplicated point: its twin is left with a
    variance of rounding size, so with a stop level far above rounding and far below the real
    gains the rank is M - 1 exactly; at tol = 0 the contract allows the last step either way --
    rank M - 1, or the twin taken with a gain within the tolerance of 0."""
    n, d, s, M, scale = 130, 3, 0.1, 200, 1.0
    ref = _reference(oracle, n, d, s, M, scale)
    sig, T, k0, _ = ref
    want, _, _, wgain, _ = numpy_pivchol(sig.astype(LD), LD(k0), 48)
    level = float(np.sqrt(wgain[20] * wgain[21]) / k0)
    assert wgain[21] < level * k0 < wgain[20]
    x, y, h, w, s, xo = _case(n, d, s, M, scale)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        q = 48
        piv, gain, rank = np.full(q, 7, dtype=np.int64), np.full(q, 7.0), np.full(1, 7, np.int64)
        Cf, resid = np.full((M, q), 7.0, order="F"), np.full(M, 7.0)
        assert _raw(engine, fit, xo, M, q, 0.0, level, piv, Cf, resid, gain, rank) == 0
        assert rank[0] == 21
        assert np.array_equal(piv[:21], want[:21]) and np.all(piv[21:] == -1)
        assert np.all(gain[:21] > level * k0) and np.all(gain[21:] == 0.0)
        assert np.all(Cf[:, 21:] == 0.0) and np.all(Cf[piv[:21], np.arange(21)] > 0)
        full = fit.pivoted_cholesky(xo, 21)
        assert np.array_equal(Cf[:, :21], full[1]) and np.array_equal(resid, full[2])
        # resid is d^(rank): the next gain is its maximum, below the level
        tol = _tolerance(ref, want[:21], 0.0, "stop level")
        assert resid.max() <= level * k0 and abs(resid.max() - float(wgain[21])) <= tol
    finally:
        fit.close()

    n, d, s, M, scale = 130, 3, 0.3, 130, 1.0
    refd = _reference(oracle, n, d, s, M, scale, 0, True)
    sig, T, k0, _ = refd
    x, y, h, w, s, xo = _case(n, d, s, M, scale, 0, True)
    tr = _ld_trace(sig[:-1, :-1], numpy_pivchol(sig[:-1, :-1].astype(LD), LD(k0), M - 1)[0], 0.0)
    smallest = min(float(np.max(t)) for t in tr[:-1])
    print("duplicated point: smallest real gain %.3g k0" % (smallest / k0))
    assert smallest >= 1e-6 * k0  # the level below stands clear of every real gain
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        var = fit.predict(xo)[1]
        piv, Cf, resid, gain = fit.pivoted_cholesky(xo, M, tol=1e-9)
        assert piv.shape == (M - 1,) and len(set(piv.tolist())) == M - 1
        assert (0 in piv) != (M - 1 in piv)  # one of the twins is taken, the other left
        if var[0] == var[-1]:  # equal bits: the tie goes to the lower index
            assert 0 in piv
        tol = _tolerance(refd, piv, 0.0, "duplicated point")
        left = M - 1 if 0 in piv else 0
        assert Cf.shape == (M, M - 1) and np.all(resid[piv] == 0.0) and abs(resid[left]) <= tol
        piv0, C0, resid0, gain0 = fit.pivoted_cholesky(xo, M, tol=0.0)
        assert np.array_equal(piv0[:M - 1], piv) and np.array_equal(gain0[:M - 1], gain)
        assert piv0.shape[0] in (M - 1, M)
        if piv0.shape[0] == M:
            assert piv0[-1] == left and 0 < gain0[-1] <= tol
        assert np.all(np.isfinite(C0)) and np.all(np.isfinite(resid0))
    finally:
        fit.close()


def test_noisy_resid_is_the_variance_after_append(engine, oracle):
    """With nugget = s^2 the variances left are those of a fit that has appended the chosen points
    with arbitrary targets.  Both are held to the closed form on Sigma_ref in long double; the
    tolerance is measured on the float64 closed form over the device's algebra."""
    n, d, s, M, scale, q = 130, 3, 0.1, 200, 1.0, 24
    ref = _reference(oracle, n, d, s, M, scale)
    sig, T, k0, cpu = ref
    x, y, h, w, s, xo = _case(n, d, s, M, scale)
    nu = s * s
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        piv, _, resid, _ = fit.pivoted_cholesky(xo, q, nugget=nu, want_factor=False)
        fit.append(xo[:, piv], np.random.RandomState(5).randn(q))
        var = fit.predict(xo)[1]
    finally:
        fit.close()
    S = sig.astype(LD)
    A = S[np.ix_(piv, piv)] + LD(nu) * np.eye(q, dtype=LD)
    closed = np.diag(S) - np.sum(S[:, piv] * _ld_solve_spd(A, S[piv, :]).T, axis=1)
    cl64 = np.diag(cpu) - np.sum(cpu[:, piv] * np.linalg.solve(
        cpu[np.ix_(piv, piv)] + nu * np.eye(q), cpu[piv, :]).T, axis=1)
    r = max(float(np.max(np.abs(cl64 - closed))), float(np.max(np.abs(cpu - sig)))) / T
    tol = MARGIN * max(r, 4 * EPS) * T
    e1, e2 = float(np.max(np.abs(resid - closed))), float(np.max(np.abs(var - closed)))
    print("r %.3g; resid error / tol %.3g, appended variance error / tol %.3g"
          % (r, e1 / tol, e2 / tol))
    assert e1 <= tol and e2 <= tol
    assert float(np.max(np.abs(resid - var))) <= 2 * tol


def test_argument_errors_write_nothing(engine):
    x, y, h, w, s, xo = _case(40, 2, 0.3, 10, 1.0)
    M = 10
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        def outs():
            return (np.full(4, 7, dtype=np.int64), np.full((M, 4), 7.0, order="F"),
                    np.full(M, 7.0), np.full(4, 7.0), np.full(1, 7, dtype=np.int64))

        bad = [dict(M=-1), dict(q=0), dict(q=-3), dict(q=M + 1), dict(nugget=-1e-3),
               dict(nugget=np.nan), dict(nugget=np.inf), dict(tol=-1e-3), dict(tol=np.nan),
               dict(tol=np.inf), dict(drop="piv"), dict(drop="gain"), dict(drop="rank"),
               dict(M=2 ** 20 + 1, q=1), dict(drop="xo")]
        for kw in bad:
            piv, Cf, resid, gain, rank = o = outs()
            a = dict(M=M, q=4, nugget=0.0, tol=0.0)
            a.update({k: v for k, v in kw.items() if k != "drop"})
            drop = kw.get("drop")
            st = _raw(engine, fit, None if drop == "xo" else xo, a["M"], a["q"], a["nugget"],
                      a["tol"], None if drop == "piv" else piv, Cf, resid,
                      None if drop == "gain" else gain, None if drop == "rank" else rank)
            assert st != 0, kw
            assert all(np.all(v == 7) for v in o), kw
        with pytest.raises(ValueError):
            fit.pivoted_cholesky(xo, 0)
        with pytest.raises(ValueError):
            fit.pivoted_cholesky(np.zeros((3, 4)), 2)
        # M = 0: rank 0 and nothing else touched but the tails
        piv, Cf, resid, gain, rank = outs()
        assert _raw(engine, fit, None, 0, 4, 0.0, 0.0, piv, Cf, resid, gain, rank) == 0
        assert rank[0] == 0 and np.all(piv == -1) and np.all(gain == 0.0)
        assert np.all(Cf == 7.0) and np.all(resid == 7.0)
        # optional outputs may be missing
        piv, Cf, resid, gain, rank = outs()
        assert _raw(engine, fit, xo, M, 4, 0.0, 0.0, piv, None, None, gain, rank) == 0
        assert rank[0] == 4 and np.array_equal(piv, fit.pivoted_cholesky(xo, 4)[0])
        # the fit is not disturbed
        assert np.all(np.isfinite(fit.predict(xo)[1]))
    finally:
        fit.close()


def _columns(x, h, w, s, xo, P, oracle=None):
    """(Sigma[:, P], diag Sigma, T): in long double from the definition, or -- with the oracle -- by
    the device's algebra in float64 (Cholesky, triangular solve, K - V V^T).  No M x M matrix."""
    if oracle is None:
        from test_gp_sample import _ld_gram
        n = x.shape[1]
        A = _ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD)
        Kox = _ld_gram(xo, x, h, w)
        cols = _ld_gram(xo, xo[:, P], h, w) - Kox @ _ld_solve_spd(A, Kox[P].T)
        diag = np.diag(_ld_gram(xo[:, :1], xo[:, :1], h, w))[0] - \
            np.sum(Kox * _ld_solve_spd(A, Kox.T).T, axis=1)
        return cols, diag, None
    from scipy.linalg import solve_triangular
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    V = solve_triangular(Lc, np.ascontiguousarray(oracle.gram_cross(x, xo, h, w)), lower=True).T
    k0 = float(np.asarray(oracle.gram(xo[:, :1], h, w, 0.0))[0, 0])
    vv = np.sum(V * V, axis=1)
    cols = np.asarray(oracle.gram_cross(xo, np.asfortranarray(xo[:, P]), h, w)) - V @ V[P].T
    return cols, k0 - vv, k0 + float(np.max(vv))


def _along(cols, diag, P, nu):
    """The recurrence along the pivots P on the columns Sigma[:, P] alone, in their precision:
    (C, d^(j) before every step and after the last)."""
    dt = cols.dtype.type
    d = np.array(diag, dtype=cols.dtype)
    Cf = np.zeros_like(cols)
    trace = []
    for j, p in enumerate(P):
        trace.append(d.copy())
        c = (cols[:, j] - Cf[:, :j] @ Cf[p, :j]) / np.sqrt(d[p] + dt(nu))
        Cf[:, j] = c
        d = d - c * c
    trace.append(d)
    return Cf, trace


def _column_errors(Cf, resid, gain, P, cols, diag, nu):
    Cl, g = Cf.astype(LD), gain.astype(LD)
    Lf = np.tril(Cl[P], -1) + np.diag(np.sqrt(g + LD(nu)))
    target = cols[P] + LD(nu) * np.eye(len(P), dtype=LD)
    return {
        "C L^T": float(np.max(np.abs(Cl @ Lf.T - cols))),
        "L L^T": float(np.max(np.abs(Lf @ Lf.T - target))),
        "resid, rowsum": float(np.max(np.abs(resid - (diag - np.sum(Cl * Cl, axis=1))))),
        "gain": float(np.max(np.abs(np.diag(Cl[P]) * np.sqrt(g + LD(nu)) - g))),
    }


@pytest.mark.parametrize("M,q,noisy", [(16384, 8, False), (16384, 8, True), (65700, 6, False)])
def test_many_row_blocks(engine, oracle, M, q, noisy):
    """The sizes at which the launches take another shape: 256-row workgroups of the column kernel
    from Mp = 16384 on, and more candidates than the selecting workgroup has threads (Mp = 65728:
    257 of them, the last finishing workgroup half padding).  Sigma does not fit a test there, and
    the contract needs only its columns at the pivots and its diagonal: both from the definition
    in long double, the tolerance measured on the same columns by the device's algebra in float64
    with the recurrence along the device's pivots."""
    n, d, s, scale = 40, 2, 0.3, 1.0
    x, y, h, w, s, xo = _case(n, d, s, M, scale)
    nu = _nu(s, noisy)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        piv, Cf, resid, gain = fit.pivoted_cholesky(xo, q, nugget=nu)
        half = fit.pivoted_cholesky(xo, q // 2, nugget=nu)
    finally:
        fit.close()
    assert piv.shape == (q,) and Cf.shape == (M, q) and np.all(np.isfinite(Cf))
    assert np.array_equal(half[0], piv[:q // 2]) and np.array_equal(half[1], Cf[:, :q // 2])
    cols, diag, _ = _columns(x, h, w, s, xo, piv)
    c64, d64, T = _columns(x, h, w, s, xo, piv, oracle)
    C64, tr64 = _along(c64, d64, piv, nu)
    g64 = np.array([t[p] for t, p in zip(tr64, piv)])
    r = max(max(_column_errors(C64, tr64[-1], g64, piv, cols, diag, nu).values()),
            float(np.max(np.abs(c64 - cols))), float(np.max(np.abs(d64 - diag)))) / T
    tol = MARGIN * max(r, 4 * EPS) * T
    errs = _column_errors(Cf, resid, gain, piv, cols, diag, nu)
    _, trace = _along(cols, diag, piv, nu)
    short = max(float(np.max(t) - t[p]) for t, p in zip(trace, piv))
    errs["resid, long double"] = float(np.max(np.abs(resid - trace[-1])))
    print("M=%d q=%d nu=%g: r %.3g; error / tol %s; greedy shortfall / tol %.3g"
          % (M, q, nu, r, {k: round(v / tol, 5) for k, v in errs.items()}, short / tol))
    assert all(e <= tol for e in errs.values()) and short <= tol
    if nu == 0.0:
        assert len(set(piv.tolist())) == q and np.all(resid[piv] == 0.0)
        assert np.all(Cf[piv][np.triu_indices(q, 1)] == 0.0)
