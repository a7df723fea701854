"""What a resident fit caches and which event drops it (the table beside bq_fit::have in
csrc/host.h, DESIGN "A fit's derived state"), pinned with twins: two fits of the same data in one
engine.  The warm one runs every consumer, then the event, then every consumer again; the cold
one runs the event and then every consumer.  After the event the two agree bit for bit on
everything: a cached result that outlives an event it should not, or a workspace that a second
use does not fully rewrite, is a difference.

d = 2 throughout, s = 0.1 (0 where a failure is wanted), n <= 130: systems of 128 or 192 rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

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

# Hessian before the LOO gradient, and after it: whichever comes first runs the products stage
ORDERS = {
    "hess_first": ("logml_hess", "loo", "loo_grad"),
    "loo_grad_first": ("loo", "loo_grad", "logml_hess"),
}


def _consumers(fit, order):
    """Every consumer of a fit, by name, in a fixed sequence that ends with `order`."""
    n = fit.n
    use = {
        "logml": lambda: fit.logml,
        "L": fit.L,
        "z": fit.z,
        "alpha": fit.alpha,
        "predict_cov": lambda: fit.predict(XO, want_cov=True),
        "predict_mean": lambda: fit.predict(XO, want_var=False)[0],
        "solve_1": lambda: fit.solve(B[:n, 0]),
        "solve_3": lambda: fit.solve(B[:n]),
        "logml_grad": fit.logml_grad,
        "logml_hess": fit.logml_hess,
        "loo": fit.loo,
        "loo_grad": fit.loo_grad,
    }
    first = [k for k in use if k not in order]
    return [(k, use[k]) for k in first + list(order)]


def _consume(fit, order):
    return {k: fn() for k, fn in _consumers(fit, order)}


def _flat(v):
    return list(v) if isinstance(v, tuple) else [v]


def _assert_same_bits(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        a, b = _flat(got[k]), _flat(want[k])
        assert len(a) == len(b), (what, k)
        for i, (u, v) in enumerate(zip(a, b)):
            if isinstance(v, np.ndarray):
                assert u.shape == v.shape and np.array_equal(u, v), \
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
