"""What a resident fit caches and which event drops it (the table beside bq_fit::have in
csrc/host.h, DESIGN "A fit's derived state"), and that its consumers leave each other alone.  Every
check on the device is exact: no kernel adds in an order that depends on timing, so a fit that has
done everything else first gives the bits of one that has not.

ROWS is the one table of consumers: every result-returning public method of engine.Fit, with the
argument sets that take another route (30 rows over 24 methods).  Pinned over it:

* the events, with twins: two fits of the same data in one engine.  The warm one runs every
  consumer, then the event, then every consumer again; the cold one runs the event and then every
  consumer.  After the event the two agree on everything: a cached result that outlives an event
  it should not, or a workspace that a second use does not fully rewrite, is a difference.  A
  failed append keeps every result, a failed refit drops every one;
* a second answer is the first (test_second_answer_is_the_first): with no event in between every
  consumer repeats its bits, whichever consumers ran in between and in whichever order -- a cached
  result that a later consumer's scratch use damaged is a difference;
* a consumer alone is the consumer after all the others
  (test_each_consumer_alone_is_the_consumer_after_all);
* dirty padding (test_dirty_padding): a call with few query points or design steps after one with
  many, other points, gives a fresh fit's first call;
* keyed caches follow their key (test_keyed_caches_follow_their_key): A, B, A for the trend's
  basis and both measures, with keys that differ in everything and in one component; after set_y
  alone every consumer asks for a refit (test_after_set_y_alone_every_consumer_asks_for_a_refit);
* two fits of different padding and dimension alternate on one context
  (test_two_fits_share_a_context).

Two tests without a device keep the table whole: every public method of engine.Fit is a row here or
in NOT_CONSUMERS, and the enum's two event masks and DESIGN's table hold every bit.

d = 2 throughout, s = 0.1 (0 where a failure is wanted), n <= 130: systems of 128 or 192 rows.  The
exceptions: the second fit of test_two_fits_share_a_context (n = 300, d = 3) and the last case of
test_second_answer_is_the_first (n = 1100: 1152 rows, the 512-wide inverses and the blocked
sweeps)."""
import os
import re
from collections import namedtuple

import numpy as np
import pytest

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D, H, S = 2, 1.3, 0.1
W = np.array([0.2, 0.25])
H2, W2 = 0.9, np.array([0.3, 0.22])
_RS = np.random.RandomState(7)
X = _RS.uniform(-3.0, 3.0, size=(D, 200))
Y = np.sin(X).sum(axis=0) + 0.1 * _RS.randn(200)
Y2 = np.cos(X).sum(axis=0) + 0.1 * _RS.randn(200)
XO = _RS.uniform(-3.2, 3.2, size=(D, 40))
XB = _RS.uniform(-3.2, 3.2, size=(D, 5))
B = _RS.randn(200, 3)

# ---- what the rows are called with (a generator of its own: the draws above stay as they were) ----
_RA = np.random.RandomState(11)
# one fixed partition into groups of 1, 7 and 64 members, below the smallest n any event leaves
_PERM = _RA.permutation(96)
GROUPS = (_PERM[:1], _PERM[1:8], _PERM[8:72])
XR = _RA.uniform(-3.2, 3.2, size=(D, 23))
# the keyed consumers' keys: (degree, center, scale) and (mu, cov), cov not diagonal
TKEY = (2, np.array([0.3, -0.2]), np.array([2.0, 1.5]))
MEAS = (np.array([0.4, -0.3]), np.array([[1.0, 0.3], [0.3, 0.8]]))

# xo: the query points, and the designs' candidates; xr: reference points of their own for the
# integrated variance; q: design steps; b: right-hand sides, (>= n, 3)
Args = namedtuple("Args", "xo xr q b groups tkey meas")
ARGS = Args(XO, XR, 5, B, GROUPS, TKEY, MEAS)

# (row, the method of engine.Fit it calls, the call).  Every tuple member a method returns is
# compared.  A new consumer is one more row: test_every_public_method_is_a_row_or_no_consumer fails
# until it is there.
ROWS = (
    ("logml", "logml", lambda f, a: f.logml),
    ("L", "L", lambda f, a: f.L()),
    ("z", "z", lambda f, a: f.z()),
    ("alpha", "alpha", lambda f, a: f.alpha()),
    ("K", "K", lambda f, a: f.K()),
    ("predict_cov", "predict", lambda f, a: f.predict(a.xo, want_cov=True)),
    ("predict_mean", "predict", lambda f, a: f.predict(a.xo, want_var=False)[0]),
    ("solve_1", "solve", lambda f, a: f.solve(a.b[:f.n, 0])),
    ("solve_3", "solve", lambda f, a: f.solve(a.b[:f.n])),
    ("logml_grad", "logml_grad", lambda f, a: f.logml_grad()),
    ("logml_hess", "logml_hess", lambda f, a: f.logml_hess()),
    ("loo", "loo", lambda f, a: f.loo()),
    ("loo_grad", "loo_grad", lambda f, a: f.loo_grad()),
    ("lgo", "lgo", lambda f, a: f.lgo(a.groups)),
    ("lgo_grad", "lgo_grad", lambda f, a: f.lgo_grad(a.groups)),
    ("predict_grad", "predict_grad", lambda f, a: f.predict_grad(a.xo)),
    ("predict_grad_mean", "predict_grad", lambda f, a: f.predict_grad(a.xo, want_var=False)),
    ("predict_dtheta", "predict_dtheta", lambda f, a: f.predict_dtheta(a.xo)),
    ("predict_dtheta_mean", "predict_dtheta",
     lambda f, a: f.predict_dtheta(a.xo, want_var=False)),
    ("sample", "sample", lambda f, a: f.sample(a.xo, S=3, seed=20240229, want_chol=True)),
    ("pivoted_cholesky", "pivoted_cholesky", lambda f, a: f.pivoted_cholesky(a.xo, a.q)),
    ("ivr_design", "ivr_design", lambda f, a: f.ivr_design(a.xo, a.q, want_scores=True)),
    ("ivr_design_xr", "ivr_design",
     lambda f, a: f.ivr_design(a.xo, a.q, xr=a.xr, want_scores=True)),
    ("trend", "trend", lambda f, a: f.trend(*a.tkey)),
    ("predict_trend", "predict_trend", lambda f, a: f.predict_trend(a.xo, *a.tkey)),
    ("predict_trend_mean", "predict_trend",
     lambda f, a: f.predict_trend(a.xo, *a.tkey, want_var=False)),
    ("integral", "integral", lambda f, a: f.integral(*a.meas, want_weights=True)),
    ("integral_design", "integral_design",
     lambda f, a: f.integral_design(a.xo, a.q, *a.meas, want_scores=True)),
    ("sq_integral", "sq_integral", lambda f, a: f.sq_integral(*a.meas, want_r=True)),
    ("sq_integral_design", "sq_integral_design",
     lambda f, a: f.sq_integral_design(a.xo, a.q, *a.meas, want_scores=True)),
)
TABLE = {k: fn for k, _, fn in ROWS}
NAMES = tuple(k for k, _, _ in ROWS)
assert len(TABLE) == len(ROWS)
# the rows whose workspaces are sized by the number of points or of design steps
SIZED = ("predict_cov", "predict_mean", "predict_grad", "predict_grad_mean", "predict_dtheta",
         "predict_dtheta_mean", "sample", "pivoted_cholesky", "ivr_design", "ivr_design_xr",
         "predict_trend", "predict_trend_mean", "integral_design", "sq_integral_design")

# The public names of engine.Fit that are no consumers: they return no result of the fit.
NOT_CONSUMERS = {
    "close",             # releases the handle
    "refit", "set_y", "append", "remove",  # the events themselves
    "refit_predict",     # an event; what it returns is compared as EVENTS' return value
    "trend_last_route",  # which route the last predict_trend took: a diagnostic, two integers
}

# The products stage (fit_prod) has three callers; whichever comes first runs it.  Every order
# ends with all five cross-validation and Hessian rows, so that the first of them is the first
# caller: the Hessian, the LOO gradient, the leave-group-out gradient.
ORDERS = {
    "hess_first": ("logml_hess", "loo", "loo_grad", "lgo", "lgo_grad"),
    "loo_grad_first": ("loo", "loo_grad", "logml_hess", "lgo", "lgo_grad"),
    "lgo_grad_first": ("lgo", "lgo_grad", "loo", "loo_grad", "logml_hess"),
}


def _consumers(fit, order, args=ARGS):
    """Every consumer of a fit, by name, in a fixed sequence that ends with `order`."""
    first = [k for k in NAMES if k not in order]
    return [(k, lambda k=k: TABLE[k](fit, args)) for k in first + list(order)]


def _consume(fit, order):
    return {k: fn() for k, fn in _consumers(fit, order)}


def _run(fit, names, args=ARGS):
    """The rows `names` on `fit`, in that sequence."""
    return {k: TABLE[k](fit, args) for k in names}


def _flat(v):
    return list(v) if isinstance(v, tuple) else [v]


def _assert_same_bits(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        a, b = _flat(got[k]), _flat(want[k])
        assert len(a) == len(b), (what, k)
        for i, (u, v) in enumerate(zip(a, b)):
            if isinstance(v, np.ndarray):
                assert isinstance(u, np.ndarray) and u.shape == v.shape and u.dtype == v.dtype, \
                    "%s: %s[%d] is %r, not %r" % (what, k, i, getattr(u, "shape", u), v.shape)
                assert np.array_equal(u, v), \
                    "%s: %s[%d] differs by %.3g" % (what, k, i, np.max(np.abs(u - v)))
            else:
                assert u == v, "%s: %s[%d] %r != %r" % (what, k, i, u, v)


# ---- the events: (points fitted first, what happens to the fit; its return value is compared) ----
def _refit(f):
    f.refit(H2, W2, S)


def _set_y_refit(f):
    f.set_y(Y2[:f.n])
    f.refit(H, W, S)


def _refit_predict(f):
    return f.refit_predict(H2, W2, S, XB)


def _refit_predict_remove(f):  # the layout carries border points: the removal is not in place
    out = f.refit_predict(H2, W2, S, XB)
    f.remove(np.arange(f.n - 2, f.n))
    return out


def _append(k):
    def event(f):
        f.append(X[:, f.n:f.n + k], Y[f.n:f.n + k])
    return event


def _remove_last(k):
    def event(f):
        f.remove(np.arange(f.n - k, f.n))
    return event


def _remove_5_50(f):
    f.remove([5, 50])


EVENTS = {
    "refit": (100, _refit),
    "set_y_refit": (100, _set_y_refit),
    "refit_predict": (100, _refit_predict),
    "refit_predict_remove_last_2": (100, _refit_predict_remove),
    "append_3_in_place": (100, _append(3)),
    "append_40_grows_small": (100, _append(40)),
    "append_70_grows_blocked": (100, _append(70)),
    "remove_last_2_in_place": (100, _remove_last(2)),
    "remove_last_10_shrinks": (130, _remove_last(10)),
    "remove_5_50_update": (100, _remove_5_50),
}


@gpu
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("name", sorted(EVENTS))
def test_warm_and_cold_twin_agree_after_the_event(engine, name, order):
    n, event = EVENTS[name]
    order = ORDERS[order]
    warm = engine.gp_fit(X[:, :n], Y[:n], H, W, S)
    cold = engine.gp_fit(X[:, :n], Y[:n], H, W, S)
    try:
        _consume(warm, order)
        got = {"event": event(warm)}
        got.update(_consume(warm, order))
        want = {"event": event(cold)}
        want.update(_consume(cold, order))
        assert warm.n == cold.n
        _assert_same_bits(got, want, name)
    finally:
        warm.close()
        cold.close()


@gpu
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_failed_append_keeps_every_result(engine, order):
    """A duplicate of an existing point at s = 0: the append raises and the fit is as it was."""
    n, order = 100, ORDERS[order]
    xn, yn = X[:, n:n + 3].copy(), Y[n:n + 3].copy()
    xn[:, -1] = X[:, n // 2]
    warm = engine.gp_fit(X[:, :n], Y[:n], H, W, 0.0)
    cold = engine.gp_fit(X[:, :n], Y[:n], H, W, 0.0)
    try:
        before = _consume(warm, order)
        for f in (warm, cold):
            with pytest.raises(np.linalg.LinAlgError):
                f.append(xn, yn)
            assert f.n == n
        after = _consume(warm, order)
        _assert_same_bits(after, before, "warm, after against before")
        _assert_same_bits(after, _consume(cold, order), "warm against cold")
    finally:
        warm.close()
        cold.close()


@gpu
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_failed_refit_drops_every_result(engine, order):
    """Every point twice: a refit at s = 0 raises, every consumer then raises, and after a good
    refit nothing of what the warm twin computed before is left."""
    order = ORDERS[order]
    x = np.concatenate([X[:, :50], X[:, :50]], axis=1)
    y = Y[:100]
    warm = engine.gp_fit(x, y, H, W, S)
    cold = engine.gp_fit(x, y, H, W, S)
    try:
        _consume(warm, order)
        for f in (warm, cold):
            with pytest.raises(np.linalg.LinAlgError):
                f.refit(H, W, 0.0)
        for k, fn in _consumers(warm, order):
            with pytest.raises(np.linalg.LinAlgError):
                fn()
        for f in (warm, cold):
            f.refit(H2, W2, S)
        _assert_same_bits(_consume(warm, order), _consume(cold, order), "after a good refit")
    finally:
        warm.close()
        cold.close()


# ---- consumers against each other, no event in between ------------------------------------------
_HALF = NAMES[len(NAMES) // 2:] + NAMES[:len(NAMES) // 2]
PAIRS = {
    "same": (NAMES, NAMES),
    "then_reversed": (NAMES, NAMES[::-1]),
    "reversed_then_rotated": (NAMES[::-1], _HALF),
}
# the larger shape: npad = 1152, M = 70, q = 4
_RL = np.random.RandomState(1100)
XL = _RL.uniform(-3.0, 3.0, size=(D, 1100))
YL = np.sin(XL).sum(axis=0) + 0.1 * _RL.randn(1100)
ARGS_L = ARGS._replace(xo=_RL.uniform(-3.2, 3.2, size=(D, 70)), q=4, b=_RL.randn(1100, 3))


@gpu
@pytest.mark.parametrize("case", sorted(PAIRS) + ["same_n1100"])
def test_second_answer_is_the_first(engine, case):
    """One fit runs every consumer in one order and, with no event in between, again in another:
    each second answer is the first, bit for bit.  What the twins cannot see, since warm and cold
    run the same sequence after the event: a cached result, served from its cache the second
    time, whose buffer another consumer used as scratch in between.  The last case is the first
    pair at n = 1100 (1152 rows: the 512-wide inverses, the blocked sweep route, wide's other
    layout), every row of the table included."""
    if case == "same_n1100":
        (o1, o2), x, y, args = PAIRS["same"], XL, YL, ARGS_L
    else:
        (o1, o2), x, y, args = PAIRS[case], X[:, :100], Y[:100], ARGS
    fit = engine.gp_fit(x, y, H, W, S)
    try:
        first = _run(fit, o1, args)
        _assert_same_bits(_run(fit, o2, args), first, case)
    finally:
        fit.close()


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_each_consumer_alone_is_the_consumer_after_all(engine, name):
    """A fresh fit that runs one consumer only against a fit that ran every other consumer first,
    in reversed table order, and this one last."""
    n = 100
    alone = engine.gp_fit(X[:, :n], Y[:n], H, W, S)
    last = engine.gp_fit(X[:, :n], Y[:n], H, W, S)
    try:
        want = _run(alone, [name])
        _run(last, [k for k in NAMES[::-1] if k != name])
        _assert_same_bits(_run(last, [name]), want, name)
    finally:
        alone.close()
        last.close()


# ---- dirty padding --------------------------------------------------------------------------------
# M = 100 (Mp = 128) with q = 12, then 40, 65 and 5 points with q = 3: other points at every size,
# all from one generator
_RP = np.random.RandomState(23)
SIZES = {}
for _m, _q in ((100, 12), (40, 3), (65, 3), (5, 3)):
    SIZES[_m] = ARGS._replace(xo=_RP.uniform(-3.2, 3.2, size=(D, _m)),
                              xr=_RP.uniform(-3.2, 3.2, size=(D, _m // 2 + 1)), q=_q)
SEQUENCES = {
    "large_to_small": (100, 40, 65, 5),
    # the workspaces grow in the middle: nothing may count on what the old ones held
    "grows_in_the_middle": (5, 100, 40, 65),
}


@pytest.fixture(scope="module")
def first_calls(engine):
    """{(row, M): that row as a fresh fit's first call at M points}, computed once."""
    out = {}
    for m, args in SIZES.items():
        for k in SIZED:
            fit = engine.gp_fit(X[:, :100], Y[:100], H, W, S)
            try:
                out[k, m] = TABLE[k](fit, args)
            finally:
                fit.close()
    return out


@gpu
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_dirty_padding(engine, first_calls, seq):
    """One fit runs every consumer that takes points or design steps at one size after the other.
    Rows M .. Mp - 1 of a sweep's workspaces, and the columns behind npad where a design keeps its
    own, then hold what the call before left there; a fresh fit's first call never sees that.
    Each answer is the fresh fit's."""
    fit = engine.gp_fit(X[:, :100], Y[:100], H, W, S)
    try:
        for m in SEQUENCES[seq]:
            got = _run(fit, SIZED, SIZES[m])
            _assert_same_bits(got, {k: first_calls[k, m] for k in SIZED}, "%s, M = %d" % (seq, m))
    finally:
        fit.close()


# ---- keyed caches ---------------------------------------------------------------------------------
_MU_B = np.array([-0.6, 0.5])
_COV_B = np.array([[0.7, -0.2], [-0.2, 1.3]])
_COV_OFF = np.array([[1.0, 0.25], [0.25, 0.8]])  # MEAS's but for the off-diagonal entry
_TREND_ROWS = ("trend", "predict_trend", "predict_trend_mean")
_KMEAN_ROWS = ("integral", "integral_design")
_SQW_ROWS = ("sq_integral", "sq_integral_design")
# (the rows that share the cache, key A, key B)
KEYED = {
    "trend_all": (_TREND_ROWS, ARGS,
                  ARGS._replace(tkey=(1, np.array([-0.4, 0.1]), np.array([1.2, 2.5])))),
    "trend_degree_alone": (_TREND_ROWS, ARGS, ARGS._replace(tkey=(1,) + TKEY[1:])),
    "kmean_all": (_KMEAN_ROWS, ARGS, ARGS._replace(meas=(_MU_B, _COV_B))),
    "kmean_one_off_diagonal": (_KMEAN_ROWS, ARGS, ARGS._replace(meas=(MEAS[0], _COV_OFF))),
    "sqw_all": (_SQW_ROWS, ARGS, ARGS._replace(meas=(_MU_B, _COV_B))),
    "sqw_one_off_diagonal": (_SQW_ROWS, ARGS, ARGS._replace(meas=(MEAS[0], _COV_OFF))),
}


def _fresh(engine, rows, args, event=None):
    fit = engine.gp_fit(X[:, :100], Y[:100], H, W, S)
    try:
        if event:
            event(fit)
        return _run(fit, rows, args)
    finally:
        fit.close()


@gpu
@pytest.mark.parametrize("case", sorted(KEYED))
def test_keyed_caches_follow_their_key(engine, case):
    """TREND, KMEAN and SQW hold one key's state each.  Asked A, B, A, a fit gives A's answer
    twice and B's once, each that of a fresh fit asked that key only; B differs from A in every
    component, or in one alone (the degree; one off-diagonal entry of the covariance, both of its
    copies).  In both sequences of the rows that share the cache, so that each of them meets the
    other key's state first.  Then new targets and a refit between A and A: the cold twin's
    bits."""
    rows, a, b = KEYED[case]
    for rows in (rows, rows[::-1]):
        want_a, want_b = _fresh(engine, rows, a), _fresh(engine, rows, b)
        for k in rows:  # the two keys are two problems: no row may answer them alike
            with pytest.raises(AssertionError):
                _assert_same_bits({k: want_a[k]}, {k: want_b[k]}, case)
        fit =engine.gp_fit(X[:, :100], Y[:100], H, W, S)
        try:
            _assert_same_bits(_run(fit, rows, a), want_a, case + ": A")
            _assert_same_bits(_run(fit, rows, b), want_b, case + ": B after A")
            _assert_same_bits(_run(fit, rows, a), want_a, case + ": A after B")
            _run(fit, rows, b)
            _set_y_refit(fit)
            _assert_same_bits(_run(fit, rows, a), _fresh(engine, rows, a, _set_y_refit),
                              case + ": A after new targets and a refit")
        finally:
            fit.close()


@gpu
def test_after_set_y_alone_every_consumer_asks_for_a_refit(engine):
    """What check_fit (fit.hip) does with a stale fit: between set_y and the next refit every
    consumer, and append and remove, raise ValueError("... refit required ...") -- KMEAN, which
    outlives set_y, included -- and the refit then leaves the cold twin's bits."""
    warm = engine.gp_fit(X[:, :100], Y[:100], H, W, S)
    cold = engine.gp_fit(X[:, :100], Y[:100], H, W, S)
    try:
        _run(warm, NAMES)
        for f in (warm, cold):
            f.set_y(Y2[:100])
        for k in NAMES:
            with pytest.raises(ValueError, match="refit required"):
                TABLE[k](warm, ARGS)
        with pytest.raises(ValueError, match="refit required"):
            warm.append(X[:, 100:103], Y[100:103])
        with pytest.raises(ValueError, match="refit required"):
            warm.remove([3])
        assert warm.n == 100
        for f in (warm, cold):
            f.refit(H, W, S)
        _assert_same_bits(_run(warm, NAMES), _run(cold, NAMES), "after set_y, refusals and refit")
    finally:
        warm.close()
        cold.close()


# ---- two fits, one context ------------------------------------------------------------------------
_R3 = np.random.RandomState(3)
X3 = _R3.uniform(-2.0, 2.0, size=(3, 300))
Y3 = np.sin(X3).sum(axis=0) + 0.1 * _R3.randn(300)
W3 = np.array([0.3, 0.35, 0.4])
ARGS3 = Args(_R3.uniform(-2.1, 2.1, size=(3, 40)), _R3.uniform(-2.1, 2.1, size=(3, 23)), 5,
             _R3.randn(300, 3), GROUPS,
             (2, np.array([0.3, -0.2, 0.1]), np.array([2.0, 1.5, 1.8])),
             (np.array([0.4, -0.3, 0.2]),
              np.array([[1.0, 0.3, -0.1], [0.3, 0.8, 0.2], [-0.1, 0.2, 0.9]])))


@gpu
def test_two_fits_share_a_context(engine):
    """P (n = 100, d = 2: 128 rows) and Q (n = 300, d = 3: 320 rows, other kernel instances)
    alternate row by row over the context's shared scratch -- the panel workspace, the mapped
    staging.  Each answer is that of a lone fit of the same data that ran the same rows with no
    other fit alive."""
    def fits():
        return (engine.gp_fit(X[:, :100], Y[:100], H, W, S), ARGS), \
            (engine.gp_fit(X3, Y3, H, W3, S), ARGS3)

    want = []
    for i in (0, 1):
        lone, args = fits()[i]
        try:
            want.append(_run(lone, NAMES, args))
        finally:
            lone.close()
    (p, pa), (q, qa) = fits()
    try:
        got = ({}, {})
        for k in NAMES:
            got[0][k] = TABLE[k](p, pa)
            got[1][k] = TABLE[k](q, qa)
        _assert_same_bits(got[0], want[0], "P beside Q")
        _assert_same_bits(got[1], want[1], "Q beside P")
    finally:
        p.close()
        q.close()


# ---- without a device: the table is complete ------------------------------------------------------
def test_every_public_method_is_a_row_or_no_consumer():
    """Every public method or property of engine.Fit is called by a row of ROWS or stands in
    NOT_CONSUMERS: a new consumer cannot arrive without joining the table."""
    from bayesian_quadrature_amd import engine as eng_mod
    public = {k for k, v in vars(eng_mod.Fit).items()
              if not k.startswith("_") and (callable(v) or isinstance(v, property))}
    assert NOT_CONSUMERS <= public, sorted(NOT_CONSUMERS - public)
    methods = {m for _, m, _ in ROWS}
    assert not methods & NOT_CONSUMERS
    assert public - NOT_CONSUMERS == methods, sorted((public - NOT_CONSUMERS) ^ methods)
    assert set(SIZED) <= set(NAMES) and all(k in NAMES for o in ORDERS.values() for k in o)


def _have_enum():
    """{name: value} of bq_fit's anonymous enum, read as text."""
    with open(os.path.join(ROOT, "bayesian-quadrature_amd", "csrc", "host.h")) as f:
        text = f.read()
    body = re.search(r"struct bq_fit : FitCore \{.*?enum : unsigned \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    out = {}
    for name, expr in re.findall(r"(\w+)\s*=\s*([^,]+),", body):
        shift = re.fullmatch(r"\s*1u\s*<<\s*(\d+)\s*", expr)
        if shift:
            out[name] = 1 << int(shift.group(1))
        else:
            out[name] = 0
            for term in expr.split("|"):
                out[name] |= out[term.strip()]
    return out


def test_event_masks_hold_every_bit():
    """FACTOR_CHANGED is every result bit, TARGETS_CHANGED all of them but DW, WIDE and KMEAN, and
    DESIGN's table of the derived state has one row per bit."""
    enum = _have_enum()
    factor, targets = enum.pop("FACTOR_CHANGED"), enum.pop("TARGETS_CHANGED")
    assert len(enum) >= 13 and {"DW", "WIDE", "KMEAN", "SQW"} <= set(enum)
    assert sorted(enum.values()) == [1 << i for i in range(len(enum))]  # one bit each, no gap
    assert factor == sum(enum.values())
    assert targets == factor & ~(enum["DW"] | enum["WIDE"] | enum["KMEAN"])
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        sec = f.read().split("## 4e.")[1].split("\n## ")[0]
    rows = re.findall(r"^\| `(\w+)` \|", sec, re.M)
    assert sorted(rows) == sorted(enum), (rows, sorted(enum))
