"""The marginal of a resident fit on the device (csrc/marginal.h; bq_gp_marginal, bq_gp_marginal_box,
bq_marginal_K, bq_marginal_K_box) against ld_marginal.py's long-double references: the cross
matrix and the prior per entry at every dimension, set of kept axes and tile seam; the posterior
mean, variance and covariance against the long-double Gram, Cholesky and substitution; exact zeros
outside a box; the bits of a fresh fit after every event and between the other consumers of the
shared workspaces, and test_gp_fit_state.py's checks over its table of consumers with marginal's
rows beside all of its rows; and every illegal argument through the four C entry points."""
import ctypes as C
import functools

import numpy as np
import pytest

import ld_marginal as lm
from ld_closed_forms import EPS, LD, MARGIN, all_normal, entry_units, integral_bar, ld_chol
from test_gp_pivchol import _ld_solve_spd
from test_gp_sample import _case, _ld_gram

pytestmark = pytest.mark.gpu

SETS = [(d, axes) for d in lm.DIMS for axes in lm.keep_sets(d)]


def _measures():
    from bayesian_quadrature_amd import measures
    return measures


def _measure_of(c):
    return (_measures().BoxMeasure(c["lo"], c["hi"]),) if c["kind"] == "box" else (c["mu"], c["cov"])


def _per_entry(engine, full, case_of):
    """Every (M, n) of the seams on one family: the cross matrix and the prior's diagonal per
    entry, a second call's bits, and NaN against zeros in the coordinates that are never read."""
    assert all_normal(full["ref"]) and all_normal(full["pdiag"])
    worst = 0.0
    for M in lm.MS:
        for n in lm.NS:
            c = case_of(M, n)
            assert all_normal(c["ref"]) and all_normal(c["pdiag"])
            args = (c["xq"], c["x"], c["h"], c["w"], c["axes"]) + _measure_of(c)
            got, pd = engine.marginal_K(*args)
            assert got.shape == (M, n) and pd.shape == (M,)
            worst = max(worst, lm.check_entries(got, c), lm.check_entries(pd, c, "pdiag", "r_p"))
            again, pd2 = engine.marginal_K(*args)
            assert np.array_equal(got, again) and np.array_equal(pd, pd2)
    return worst


@pytest.mark.parametrize("d,axes", SETS)
@pytest.mark.parametrize("fam", lm.GAUSS_FAMILIES)
def test_gaussian_cross_and_prior_per_entry(engine, fam, d, axes):
    worst = _per_entry(engine, lm.gauss_case(fam, d, axes),
                       lambda M, n: lm.gauss_case(fam, d, axes, M, n))
    c = lm.gauss_case(fam, d, axes)
    print("gauss %s d=%d keep %s: r %.1f eps, r_p %.1f eps, smallest entry %.3g, worst error / bar "
          "%.3g" % (fam, d, axes, c["r"] / EPS, c["r_p"] / EPS, float(c["ref"].min()), worst))


@pytest.mark.parametrize("d,axes", SETS)
def test_box_cross_and_prior_per_entry(engine, d, axes):
    worst = _per_entry(engine, lm.box_case(d, axes), lambda M, n: lm.box_case(d, axes, M, n))
    c = lm.box_case(d, axes)
    assert c["live"].sum() not in (0, c["live"].size)      # inside, on a face, and outside
    print("box d=%d keep %s: r %.1f eps, r_p %.1f eps, worst error / bar %.3g"
          % (d, axes, c["r"] / EPS, c["r_p"] / EPS, worst))


@pytest.mark.parametrize("d", lm.DIMS)
def test_unread_coordinates_are_never_read(engine, d):
    """bq_marginal_K with NaN in the integrated axes' rows of xq gives the bits it gives with
    zeros there (engine.marginal_K itself scatters NaN)."""
    axes = lm.keep_sets(d)[-1]
    for c in (lm.gauss_case("corr", d, axes, 65, 257), lm.box_case(d, axes, 65, 257)):
        S, I = lm.split(d, axes)
        m = _measure_of(c)
        name, margs = ("_box", (m[0].lo, m[0].hi)) if c["kind"] == "box" else ("", m)
        keep = np.zeros(d, dtype=np.int32)
        keep[S] = 1
        outs = []
        for fill in (np.nan, 0.0):
            xq = np.full((d, 65), fill, order="F")
            xq[S] = c["xq"]
            out, pd = np.empty((65, 257), order="F"), np.empty(65)
            st = getattr(engine._lib, "bq_marginal_K" + name)(
                engine._ctx, _p(xq), 65, _p(c["x"]), 257, d, c["h"], _p(c["w"]),
                keep.ctypes.data_as(C.POINTER(C.c_int32)),
                *[_p(np.asfortranarray(a, dtype=np.float64)) for a in margs], _p(out), _p(pd))
            assert st == 0
            outs.append((out, pd))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        assert np.array_equal(outs[0][0], engine.marginal_K(
            c["xq"], c["x"], c["h"], c["w"], axes, *m)[0])


def _p(a, t=C.POINTER(C.c_double)):
    return None if a is None else a.ctypes.data_as(t)


# ---- the posterior ----------------------------------------------------------------------------
S_OF = {65: 0.1, 130: 0.1, 70: 0.05}          # s as in test_gp_zdesign.CASES
POST = [(65, 2), (130, 3), (70, 5), (65, 8)]
POST_M = (1, 70, 200)


def _post_measure(kind, d):
    if kind == "box":
        return dict(kind="box", lo=np.full(d, -2.0), hi=np.full(d, 3.0))
    mu = np.array([0.25 * (-1) ** k for k in range(d)])
    return dict(kind="gauss", mu=mu, cov=np.asfortranarray(1.5 ** 2 * (0.7 * np.eye(d) + 0.3)))


def _post_queries(kind, d, axes, M):
    xq = np.random.RandomState(40 + d + len(axes)).uniform(-2.0, 3.0, (len(axes), M))
    if kind == "box":      # inside, on a face, outside
        for i in range(M):
            if i % 3 == 1:
                xq[i % len(axes), i] = 3.0
            elif i % 3 == 2:
                xq[i % len(axes), i] = 3.5
    return xq


@functools.lru_cache(maxsize=None)
def _posterior(oracle, kind, n, d, axes):
    """The long-double posterior at the 200 query points (the first M are a case's) and the
    float64 restatement on the oracle's algebra, with the scales of the three bars."""
    from scipy.linalg import solve_triangular
    x, y, h, w, s, _ = _case(n, d, S_OF[n], 1, 1.0)
    m = _post_measure(kind, d)
    xq = _post_queries(kind, d, axes, max(POST_M))
    if kind == "box":
        c, P = lm.ld_marg_box(xq, x, h, w, axes, m["lo"], m["hi"])
        c64, P64 = lm.f64_marg_box(xq, x, h, w, axes, m["lo"], m["hi"])
    else:
        c, P = lm.ld_marg_gauss(xq, x, h, w, axes, m["mu"], m["cov"])
        c64, P64 = lm.f64_marg_gauss(xq, x, h, w, axes, m["mu"], m["cov"])
    A = _ld_gram(x, x, h, w) + LD(s) ** 2 * np.eye(n, dtype=LD)
    alpha = _ld_solve_spd(A, y.astype(LD))
    Lf = ld_chol(A)
    V = np.array(c)
    for j in range(n):
        V[:, j] = (V[:, j] - V[:, :j] @ Lf[j, :j]) / Lf[j, j]
    Lc = np.linalg.cholesky(oracle.gram(x, h, w, s))
    V64 = solve_triangular(Lc, np.ascontiguousarray(c64.T), lower=True).T
    z = solve_triangular(Lc, y, lower=True)
    pd = np.diag(P).astype(np.float64)
    out = dict(x=x, y=y, h=h, w=w, s=s, xq=xq, m=m,
               mean=c @ alpha, cov=P - V @ V.T, mean64=V64 @ z, cov64=P64 - V64 @ V64.T,
               ms=(np.abs(c) @ np.abs(alpha)).astype(np.float64), vs=pd,
               cs=np.sqrt(np.outer(pd, pd)))
    return out


def _r(got, ref, scale):
    """The largest error in units of the scale, over the entries whose scale is not zero (where
    it is zero -- outside a box -- the reference is zero and so must the result be)."""
    got, ref = np.asarray(got), np.asarray(ref)
    live = scale > 0
    assert not np.any(got[~live])
    if not live.any():
        return 0.0
    return float(np.max(np.abs(got[live].astype(LD) - ref[live]) / scale[live]))


@pytest.mark.parametrize("nk", (1, 2))
@pytest.mark.parametrize("n,d", POST)
@pytest.mark.parametrize("kind", ("gauss", "box"))
def test_posterior_against_long_double(engine, oracle, kind, n, d, nk):
    axes = (d - 1,) if nk == 1 else (0, d - 1)
    if nk == 2 and d == 2:
        axes = (0,)       # d = 2 keeps one axis either way: the other one
    p = _posterior(oracle, kind, n, d, axes)
    m = p["m"]
    meas = (_measures().BoxMeasure(m["lo"], m["hi"]),) if kind == "box" else (m["mu"], m["cov"])
    fit = engine.gp_fit(p["x"], p["y"], p["h"], p["w"], p["s"])
    try:
        for M in POST_M:
            xq = p["xq"][:, :M]
            ms, vs, cs = p["ms"][:M], p["vs"][:M], p["cs"][:M, :M]
            ref_v = np.diag(p["cov"])[:M]
            rm = _r(p["mean64"][:M], p["mean"][:M], ms)
            rv = _r(np.diag(p["cov64"])[:M], ref_v, vs)
            rc = _r(p["cov64"][:M, :M], p["cov"][:M, :M], cs)
            bm, bv, bc = (MARGIN * max(r, 4 * EPS) for r in (rm, rv, rc))
            mean, var, cov = fit.marginal(xq, axes, *meas, want_cov=True)
            em, ev = _r(mean, p["mean"][:M], ms), _r(var, ref_v, vs)
            ec = _r(cov, p["cov"][:M, :M], cs)
            print("%s n=%d d=%d keep %s M=%d: r mean %.3g var %.3g cov %.3g; error / bar mean %.3g "
                  "var %.3g cov %.3g" % (kind, n, d, axes, M, rm, rv, rc, em / bm, ev / bv, ec / bc))
            assert em <= bm and ev <= bv and ec <= bc
            # the covariance is symmetric, and its diagonal is var
            assert np.array_equal(cov, cov.T)
            assert _r(np.diag(cov), var, vs) <= 2 * bv
            # mean and var without cov: the sweep's bits; the mean-only route within the bar
            m2, v2, _ = fit.marginal(xq, axes, *meas)
            assert np.array_equal(m2, mean) and np.array_equal(v2, var)
            m1 = fit.marginal(xq, axes, *meas, want_var=False)[0]
            assert _r(m1, p["mean"][:M], ms) <= bm
            if kind == "box":
                out = ms == 0
                assert out.sum() == M // 3 and not np.any(cov[out]) and not np.any(cov[:, out])
                assert not np.any(m1[out])
    finally:
        fit.close()


def test_one_axis_takes_a_vector(engine):
    x, y, h, w, s, _ = _case(65, 3, 0.1, 1, 1.0)
    m = _post_measure("gauss", 3)
    q = np.linspace(-2.0, 2.0, 7)
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        a = fit.marginal(q, [1], m["mu"], m["cov"])
        b = fit.marginal(q[None, :], (1,), m["mu"], m["cov"])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] is None
        # two axes in either order: the rows follow the axes
        q2 = np.vstack([q, q[::-1]])
        c = fit.marginal(q2, [0, 2], m["mu"], m["cov"])
        e = fit.marginal(q2[::-1], [2, 0], m["mu"], m["cov"])
        assert np.array_equal(c[0], e[0]) and np.array_equal(c[1], e[1])
        assert fit.marginal(np.empty((1, 0)), [1], m["mu"], m["cov"])[0].shape == (0,)
        with pytest.raises(ValueError):
            fit.marginal(q, [1], _measures().GaussianMixture([1.0], [[0.0] * 3], [np.eye(3)]))
        with pytest.raises(ValueError):
            engine.marginal_K(q, x, h, w, [1],
                              _measures().GaussianMixture([1.0], [[0.0] * 3], [np.eye(3)]))
        for bad in ([], [0, 1, 2], [3], [0, 0]):
            with pytest.raises(ValueError):
                fit.marginal(np.zeros((len(bad), 2)), bad, m["mu"], m["cov"])
    finally:
        fit.close()


def test_points_past_two_to_the_eighteen_doubles(engine):
    """The mean-only routes take any M: d M = 2^18 + 6 doubles of query points come in through one
    staging launch whose grid is capped, and the call gives the bits of the same points in two
    halves -- marginal's and, through the same staging, predict's (which lost every point past
    2^18 doubles before)."""
    x, y, h, w, s, _ = _case(65, 2, 0.1, 1, 1.0)
    m = _post_measure("gauss", 2)
    M = (1 << 17) + 3
    rs = np.random.RandomState(3)
    q, xo = rs.uniform(-2.0, 2.0, M), np.asfortranarray(rs.uniform(-2.0, 2.0, (2, M)))
    fit = engine.gp_fit(x, y, h, w, s)
    try:
        whole = fit.marginal(q, [0], m["mu"], m["cov"], want_var=False)[0]
        halves = [fit.marginal(q[a:b], [0], m["mu"], m["cov"], want_var=False)[0]
                  for a, b in ((0, M // 2), (M // 2, M))]
        assert np.array_equal(whole, np.concatenate(halves)) and np.any(whole[-8:] != 0.0)
        whole = fit.predict(xo, want_var=False)[0]
        halves = [fit.predict(np.asfortranarray(xo[:, a:b]), want_var=False)[0]
                  for a, b in ((0, M // 2), (M // 2, M))]
        assert np.array_equal(whole, np.concatenate(halves))
    finally:
        fit.close()


# ---- state --------------------------------------------------------------------------------------
def _same(a, b):
    return all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(a, b))


def _state_case():
    x, y, h, w, s, xo = _case(130, 3, 0.1, 40, 1.0)
    m = _post_measure("gauss", 3)
    box = _measures().BoxMeasure(np.full(3, -2.0), np.full(3, 3.0))
    xq = _post_queries("box", 3, (0, 2), 70)
    return x, y, h, w, s, xo, m["mu"], m["cov"], box, xq


def _marg(f, c):
    x, y, h, w, s, xo, mu, cov, box, xq = c
    return f.marginal(xq, (0, 2), mu, cov, want_cov=True) + f.marginal(xq, (0, 2), box) + \
        f.marginal(xq[0], (1,), mu, cov, want_var=False)


def test_marginal_between_the_other_consumers(engine):
    """marginal shares wV, wV2, wx and wout with predict, pivoted_cholesky and sample, and the
    fit with integral: each of them after a marginal has the bits it has on a fresh fit, and so has
    marginal after each of them."""
    c = _state_case()
    x, y, h, w, s, xo, mu, cov, box, xq = c
    others = [("predict", lambda f: f.predict(xo, want_cov=True)),
              ("integral", lambda f: f.integral(mu, cov, want_weights=True)),
              ("pivoted_cholesky", lambda f: f.pivoted_cholesky(xo, 8)),
              ("sample", lambda f: f.sample(xo, 3, seed=5))]

    def fresh(call):
        f = engine.gp_fit(x, y, h, w, s)
        try:
            return call(f)
        finally:
            f.close()

    def flat(v):
        return [np.asarray(u) for u in (v if isinstance(v, tuple) else (v,)) if u is not None]

    want_m = fresh(lambda f: _marg(f, c))
    f = engine.gp_fit(x, y, h, w, s)
    try:
        for name, call in others:
            want = flat(fresh(call))
            assert _same(_marg(f, c), want_m), name
            got = flat(call(f))
            assert len(got) == len(want) and _same(got, want), name
            assert _same(_marg(f, c), want_m), name
    finally:
        f.close()


def test_marginal_follows_the_events(engine):
    c = _state_case()
    x, y, h, w, s, xo, mu, cov, box, xq = c
    y2 = np.cos(y) + 0.3
    rs = np.random.RandomState(11)
    xn, yn = np.asfortranarray(rs.uniform(-3, 3, size=(3, 5))), rs.randn(5)
    idx = np.array([3, 64, 100])
    keep = np.setdiff1d(np.arange(130), idx)
    events = [("set_y", lambda f: (f.set_y(y2), f.refit(h, w, s)), (x, y2, h, w, s)),
              ("refit", lambda f: f.refit(1.1 * h, 0.9 * w, s), (x, y, 1.1 * h, 0.9 * w, s)),
              ("append", lambda f: f.append(xn, yn),
               (np.asfortranarray(np.hstack([x, xn])), np.concatenate([y, yn]), h, w, s)),
              ("remove", lambda f: f.remove(idx),
               (np.asfortranarray(x[:, keep]), y[keep], h, w, s))]
    for name, ev, data in events:
        warm, cold = engine.gp_fit(x, y, h, w, s), engine.gp_fit(x, y, h, w, s)
        fresh = engine.gp_fit(*data)
        try:
            before = _marg(warm, c)
            ev(warm), ev(cold)
            a, b = _marg(warm, c), _marg(cold, c)
            assert _same(a, b) and not _same(a, before), name
            if name in ("set_y", "refit"):     # the same data in the same order: a fresh fit's bits
                assert _same(a, _marg(fresh, c)), name
        finally:
            warm.close(), cold.close(), fresh.close()


# ---- marginal's rows of the table of consumers (test_gp_fit_state.py) ---------------------------
# engine.Fit inherits ``marginal`` from engine.FitViews, so the table there, which is over Fit's own
# methods, stands as it is; its checks are run here with marginal's two rows beside all of its rows.
import test_gp_fit_state as fs  # noqa: E402

MROWS = {
    "marginal_cov": lambda f, a: f.marginal(a.xo[0], [0], *a.meas, want_cov=True),
    "marginal_mean": lambda f, a: f.marginal(a.xo[-1], [f.d - 1], *a.meas, want_var=False)[0],
    "marginal_box": lambda f, a: f.marginal(a.xo[0], [0], _measures().BoxMeasure(
        np.full(f.d, -2.0), np.full(f.d, 2.5))),
}


def _mrun(fit, args=fs.ARGS, tag=""):
    return {k + tag: fn(fit, args) for k, fn in MROWS.items()}


def _all(fit, order=fs.ORDERS["hess_first"], args=fs.ARGS):
    """marginal's rows, every row of the table, marginal's rows again."""
    out = _mrun(fit, args, ":first")
    out.update(fs._consume(fit, order) if args is fs.ARGS else fs._run(fit, fs.NAMES, args))
    out.update(_mrun(fit, args, ":last"))
    return out


@pytest.mark.parametrize("name", sorted(fs.EVENTS))
def test_warm_and_cold_twin_agree_after_the_event(engine, name):
    n, event = fs.EVENTS[name]
    warm = engine.gp_fit(fs.X[:, :n], fs.Y[:n], fs.H, fs.W, fs.S)
    cold = engine.gp_fit(fs.X[:, :n], fs.Y[:n], fs.H, fs.W, fs.S)
    try:
        before = _all(warm)
        event(warm), event(cold)
        got, want = _all(warm), _all(cold)
        fs._assert_same_bits(got, want, name)
        for k in MROWS:    # the event changed the answer, and the last answer is the first
            with pytest.raises(AssertionError):
                fs._assert_same_bits({k: got[k + ":first"]}, {k: before[k + ":first"]}, name)
            fs._assert_same_bits({k: got[k + ":last"]}, {k: got[k + ":first"]}, name)
    finally:
        warm.close(), cold.close()


@pytest.mark.parametrize("case", ("n100", "n1100"))
def test_second_answer_is_the_first_and_a_fresh_fit_s(engine, case):
    x, y, args = (fs.X[:, :100], fs.Y[:100], fs.ARGS) if case == "n100" else (fs.XL, fs.YL, fs.ARGS_L)
    fit, alone = engine.gp_fit(x, y, fs.H, fs.W, fs.S), engine.gp_fit(x, y, fs.H, fs.W, fs.S)
    try:
        want = _mrun(alone, args)
        got = _all(fit, args=args)
        for tag in (":first", ":last"):
            fs._assert_same_bits({k: got[k + tag] for k in MROWS}, want, case + tag)
        # and every row of the table between them is that row on the fit that ran marginal once
        fs._assert_same_bits({k: got[k] for k in fs.NAMES}, fs._run(alone, [
            k for k in got if k in fs.NAMES], args), case)
    finally:
        fit.close(), alone.close()


@pytest.mark.parametrize("seq", sorted(fs.SEQUENCES))
def test_dirty_padding(engine, seq):
    """marginal at one size after the other, between the table's sized rows at that size: each
    answer is a fresh fit's first call."""
    fit = engine.gp_fit(fs.X[:, :100], fs.Y[:100], fs.H, fs.W, fs.S)
    try:
        for m in fs.SEQUENCES[seq]:
            fresh = engine.gp_fit(fs.X[:, :100], fs.Y[:100], fs.H, fs.W, fs.S)
            try:
                want = _mrun(fresh, fs.SIZES[m])
            finally:
                fresh.close()
            fs._run(fit, fs.SIZED, fs.SIZES[m])
            fs._assert_same_bits(_mrun(fit, fs.SIZES[m]), want, "%s, M = %d" % (seq, m))
    finally:
        fit.close()


def test_after_set_y_alone_marginal_asks_for_a_refit(engine):
    fit = engine.gp_fit(fs.X[:, :100], fs.Y[:100], fs.H, fs.W, fs.S)
    try:
        _mrun(fit)
        fit.set_y(fs.Y2[:100])
        for k, fn in MROWS.items():
            with pytest.raises(ValueError, match="refit required"):
                fn(fit, fs.ARGS)
    finally:
        fit.close()


def test_two_fits_share_a_context(engine):
    p = engine.gp_fit(fs.X[:, :100], fs.Y[:100], fs.H, fs.W, fs.S)
    q = engine.gp_fit(fs.X3, fs.Y3, fs.H, fs.W3, fs.S)
    try:
        want = (_mrun(p, fs.ARGS), _mrun(q, fs.ARGS3))
        for _ in range(2):
            got = (_mrun(p, fs.ARGS), _mrun(q, fs.ARGS3))
            fs._assert_same_bits(got[0], want[0], "P beside Q")
            fs._assert_same_bits(got[1], want[1], "Q beside P")
    finally:
        p.close(), q.close()


# ---- arguments ----------------------------------------------------------------------------------
def test_argument_errors_write_nothing(engine):
    """Every illegal argument of include/bqhip.h through the four C entry points: BQ_ERR_BAD_ARG,
    and poisoned outputs untouched."""
    from bayesian_quadrature_amd import _lib
    x, y, h, w, s, _ = _case(40, 2, 0.3, 1, 1.0)
    d, n, M = 2, 40, 5
    i32 = C.POINTER(C.c_int32)
    lo, hi = np.array([-1.0, -2.0]), np.array([1.0, 0.5])
    mu, cov = np.array([0.1, -0.2]), np.asfortranarray([[1.0, 0.3], [0.3, 2.0]])
    keep = np.array([1, 0], dtype=np.int32)
    xq = np.asfortranarray(np.vstack([np.linspace(-0.5, 0.5, M), np.full(M, np.nan)]))

    def edit(a, idx, v):
        b = np.array(a, dtype=np.float64, order="F")
        b[idx] = v
        return b

    off = np.sqrt(0.2) * w[0] * w[1]
    bad_gauss = [(None, cov), (mu, None), (edit(mu, 0, np.nan), cov), (mu, edit(cov, (1, 1), np.inf)),
                 (mu, edit(cov, (0, 0), -10.0)),                              # W + Sigma fails
                 (mu, np.asfortranarray(-0.6 * np.diag(w ** 2))),             # only W + 2 Sigma fails
                 (mu, edit(cov, (0, 1), 0.31)),                               # not symmetric
                 (mu, np.asfortranarray(np.diag([-1e-3 * w[0] ** 2, 1.0]))),  # Sigma_SS fails alone
                 # W + Sigma, W + 2 Sigma and Sigma_SS factor; W_I + Sigma_c = -19 w_1^2 does not
                 (mu, np.asfortranarray([[0.01 * w[0] ** 2, off], [off, 0.0]]))]
    bad_box = [(None, hi), (lo, None), (edit(lo, 1, np.nan), hi), (lo, edit(hi, 0, np.inf)),
               (lo, edit(hi, 1, -2.0)), (lo, edit(hi, 1, -3.0))]
    bad_keep = [None, np.array([1, 1], dtype=np.int32), np.array([0, 0], dtype=np.int32),
                np.array([2, 0], dtype=np.int32), np.array([-1, 0], dtype=np.int32)]
    bad_xq = [None, edit(xq, (0, 3), np.nan), edit(xq, (0, 0), np.inf)]
    lib, ctx = engine._lib, engine._ctx
    fit = engine.gp_fit(x, y, h, w, s)

    def call(name, margs, kp, q, nq=M, outs=True):
        """(status of the fit's entry point, of the host arrays' one, every output untouched)"""
        me, va, co = np.full(M, 7.0), np.full(M, 7.0), np.full((M, M), 7.0, order="F")
        out, pd = np.full((M, n), 7.0, order="F"), np.full(M, 7.0)
        o = (_p(me), _p(va), _p(co)) if outs else (None, None, None)
        s1 = getattr(lib, "bq_gp_marginal" + name)(ctx, fit._handle(), _p(kp, i32), *margs, _p(q),
                                                   nq, *o)
        o = (_p(out), _p(pd)) if outs else (None, None)
        s2 = getattr(lib, "bq_marginal_K" + name)(ctx, _p(q), nq, _p(x), n, d, h, _p(w),
                                                  _p(kp, i32), *margs, *o)
        clean = all(np.all(a == 7) for a in (me, va, co, out, pd))
        return s1, s2, clean

    try:
        good = {"": (_p(mu), _p(cov)), "_box": (_p(lo), _p(hi))}
        for name in good:
            assert call(name, good[name], keep, xq)[:2] == (0, 0)
            for kp in bad_keep:
                assert call(name, good[name], kp, xq) == (_lib.BQ_ERR_BAD_ARG,) * 2 + (True,), kp
            for q in bad_xq:
                assert call(name, good[name], keep, q) == (_lib.BQ_ERR_BAD_ARG,) * 2 + (True,)
            assert call(name, good[name], keep, xq, -1) == (_lib.BQ_ERR_BAD_ARG,) * 2 + (True,)
            assert call(name, good[name], keep, xq, M, False)[:2] == (_lib.BQ_ERR_BAD_ARG,) * 2
            assert call(name, good[name], keep, None, 0) == (0, 0, True)   # M = 0: nothing written
        for a, b in bad_gauss:
            assert call("", (_p(a), _p(b)), keep, xq) == (_lib.BQ_ERR_BAD_ARG,) * 2 + (True,), (a, b)
        for a, b in bad_box:
            assert call("_box", (_p(a), _p(b)), keep, xq) == (_lib.BQ_ERR_BAD_ARG,) * 2 + (True,)
        # the fit is not disturbed
        assert np.all(np.isfinite(fit.marginal(xq[0], [0], mu, cov)[1]))
    finally:
        fit.close()
