"""CPU tests of the host plumbing of appended observations: gp.GP.append over a stub engine
whose fit records its calls, and BQ.add_observation over the oracle-backed engine double (whose
fit has no ``append``: the drop-and-refit route)."""
import numpy as np
import pytest

from engine_double import EngineDouble, FitDouble


class RecordingFit(FitDouble):
    """FitDouble with an ``append`` that refits the grown data (numpy stands in for the device)."""
    fail_with = None

    def __init__(self, o, x, y, h, w, s, log):
        self.log = log
        log.append(("fit", np.size(y)))
        FitDouble.__init__(self, o, x, y, h, w, s)

    def refit(self, h, w, s):
        self.log.append(("refit", (float(h), float(np.atleast_1d(w)[0]), float(s))))
        FitDouble.refit(self, h, w, s)

    def append(self, x_new, y_new):
        self.log.append(("append", np.size(y_new)))
        if self.fail_with is not None:
            raise self.fail_with
        self.x = np.concatenate([np.ravel(self.x), np.ravel(x_new)])
        self.y = np.concatenate([self.y, np.ravel(y_new)])
        self.n = self.y.shape[0]
        self._L, self._alpha, self.logml = self.o.gp_fit(self.x, self.y, self.h, self.w, self.s)

    def logml_grad(self):
        self.log.append(("grad", self.n))
        return np.zeros(3)

    def close(self):
        self.log.append(("close", self.n))


class NoAppendFit(RecordingFit):
    append = property()  # hasattr(fit, "append") is False


class RecordingEngine(EngineDouble):
    fit_class = RecordingFit

    def __init__(self, o):
        EngineDouble.__init__(self, o)
        self.log = []

    def gp_fit(self, x, y, h, w, s=0.0):
        return self.fit_class(self.o, x, y, h, w, s, self.log)


@pytest.fixture
def stub(oracle):
    from bayesian_quadrature_amd import engine as eng_mod
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng = RecordingEngine(oracle)
    eng_mod.set_engine(eng, 0)
    yield eng
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _data(n=30, seed=5):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-4, 4, size=n)
    return x, np.sin(x) + 0.1 * rs.randn(n)


def _gp(x, y):
    from bayesian_quadrature_amd import gp
    return gp.GP(gp.GaussianKernel(1.2, 0.8), x, y, s=0.1)


def _calls(eng, name):
    return [c for c in eng.log if c[0] == name]


def test_append_grows_the_fit_once_and_keeps_it(stub, oracle):
    x, y = _data()
    g = _gp(x[:25], y[:25])
    g.log_lh
    fit = g._fit
    g.append(x[25:], y[25:])
    assert g._fit is fit and _calls(stub, "append") == [("append", 5)]
    assert not _calls(stub, "close") and len(_calls(stub, "fit")) == 1
    assert np.array_equal(g.x, x) and np.array_equal(g.y, y)
    L, a, lm = oracle.gp_fit(x, y, 1.2, 0.8, 0.1)
    assert g.log_lh == lm and np.array_equal(g.Lxx, L) and np.array_equal(g.inv_Kxx_y, a)
    assert len(_calls(stub, "fit")) == 1 and len(_calls(stub, "refit")) == 1
    g.append(1.5, 0.3)  # scalars, as add_observation passes them
    assert g._fit is fit and g.x.shape == (31,) and _calls(stub, "append")[-1] == ("append", 1)


def test_append_clears_the_memo(stub):
    x, y = _data()
    g = _gp(x[:25], y[:25])
    L0, lm0, g0 = g.Lxx, g.log_lh, g.dloglh_dtheta
    assert g.Lxx is L0 and len(_calls(stub, "grad")) == 1
    g.append(x[25:], y[25:])
    assert g._memoized == {}
    assert g.Lxx.shape == (30, 30) and g.log_lh != lm0
    g.dloglh_dtheta
    assert _calls(stub, "grad") == [("grad", 25), ("grad", 30)]


def test_append_without_a_fit_takes_the_old_route(stub):
    x, y = _data()
    g = _gp(x[:25], y[:25])
    g.append(x[25:], y[25:])  # never fitted
    assert g._fit is None and not stub.log
    assert np.array_equal(g.x, x) and np.array_equal(g.y, y)
    g.log_lh
    assert stub.log[0] == ("fit", 30) and not _calls(stub, "append")


def test_append_with_pending_parameters_drops_the_fit(stub, oracle):
    x, y = _data()
    g = _gp(x[:25], y[:25])
    g.log_lh
    g.set_param("w", 0.5)  # pending: the resident factor belongs to w = 0.8
    g.append(x[25:], y[25:])
    assert g._fit is None and _calls(stub, "close") == [("close", 25)]
    assert not _calls(stub, "append")
    assert g.log_lh == oracle.gp_fit(x, y, 1.2, 0.5, 0.1)[2]
    assert [c for c in stub.log if c[0] == "fit"] == [("fit", 25), ("fit", 30)]


def test_append_on_a_fit_without_append_drops_it(stub, oracle):
    stub.fit_class = NoAppendFit
    x, y = _data()
    g = _gp(x[:25], y[:25])
    g.log_lh
    assert not hasattr(g._fit, "append")
    g.append(x[25:], y[25:])
    assert g._fit is None and _calls(stub, "close") == [("close", 25)]
    assert g.log_lh == oracle.gp_fit(x, y, 1.2, 0.8, 0.1)[2]


def test_linalg_error_leaves_the_gp_as_it_was(stub):
    x, y = _data()
    g = _gp(x[:25], y[:25])
    L0, lm0 = g.Lxx, g.log_lh
    fit = g._fit
    fit.fail_with = np.linalg.LinAlgError("not positive definite")
    with pytest.raises(np.linalg.LinAlgError):
        g.append(x[25:], y[25:])
    assert g._fit is fit and np.array_equal(g.x, x[:25]) and np.array_equal(g.y, y[:25])
    assert g.Lxx is L0 and g.log_lh == lm0 and not _calls(stub, "close")
    # any other engine error: the data grow, the fit is rebuilt on its next use
    fit.fail_with = RuntimeError("device lost")
    g.append(x[25:], y[25:])
    assert g._fit is None and np.array_equal(g.x, x)
    fit.fail_with = None


def test_append_rejects_shapes_as_the_setters_do(stub):
    x, y = _data()
    g = _gp(x[:25], y[:25])
    g.log_lh
    with pytest.raises(ValueError):
        g.append(np.zeros((2, 2)), np.zeros(4))
    with pytest.raises(ValueError):
        g.append(np.zeros(3), np.zeros((3, 1)))
    with pytest.raises(ValueError):
        g.append(np.zeros(3), np.zeros(2))
    g.append(np.empty(0), np.empty(0))  # nothing to add
    assert g.x.shape == (25,) and not _calls(stub, "append") and not _calls(stub, "close")


def _bq(pkg, x, l):
    return pkg.BQ(x, l, kernel=pkg.GaussianKernel, n_candidate=10, x_mean=0.0, x_var=10.0,
                  candidate_thresh=0.5, optim_method="L-BFGS-B")


@pytest.mark.parametrize("engine_kind", ["double", "recording"])
def test_add_observation_same_state_as_a_fresh_object(oracle, stub, engine_kind):
    """add_observation (the branch that adds a point) leaves the samples, the candidates and
    both GPs as an object built from scratch on the grown data under the same np.random state
    does: with the engine double (no Fit.append: the old route) and with a fit that appends."""
    import bayesian_quadrature_amd as pkg
    from bayesian_quadrature_amd import engine as eng_mod
    if engine_kind == "double":
        eng_mod.set_engine(EngineDouble(oracle), 0)
    x = np.linspace(-5, 5, 9)
    l = np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi)
    ptl, pl = (15, 2, 0), (0.2, 1.3, 0)
    np.random.seed(8728)
    bq = _bq(pkg, x, l)
    bq.init(params_tl=ptl, params_l=pl)
    bq.gp_log_l.log_lh  # the resident fit exists, as after choose_next
    gp_log_l = bq.gp_log_l
    state = np.random.get_state()
    x_a, l_a = 0.61, float(np.exp(-0.5 * 0.61 ** 2) / np.sqrt(2 * np.pi))
    bq.add_observation(x_a, l_a)
    assert bq.gp_log_l is gp_log_l and bq.ns == 10
    if engine_kind == "recording":
        assert _calls(stub, "append") == [("append", 1)]
    np.random.set_state(state)
    ref = _bq(pkg, np.append(x, x_a), np.append(l, l_a))
    ref.init(params_tl=ptl, params_l=pl)
    for name in ("x_s", "l_s", "tl_s", "x_c", "l_c", "x_sc", "l_sc"):
        assert np.array_equal(getattr(bq, name), getattr(ref, name)), name
    assert (bq.ns, bq.nc, bq.nsc) == (ref.ns, ref.nc, ref.nsc)
    assert np.array_equal(bq.gp_log_l.x, ref.gp_log_l.x)
    assert np.array_equal(bq.gp_log_l.y, ref.gp_log_l.y)
    assert np.array_equal(bq.gp_log_l.params, ref.gp_log_l.params)
    assert np.array_equal(bq.gp_log_l.jitter, np.zeros(10))
    assert np.array_equal(bq.gp_l.x, ref.gp_l.x) and np.array_equal(bq.gp_l.y, ref.gp_l.y)
    assert bq.gp_log_l.log_lh == ref.gp_log_l.log_lh
    assert bq.Z_mean() == ref.Z_mean()
    # the merge branch is the old code: a new log-GP object
    bq.add_observation(x_a + 0.1, l_a)
    assert bq.ns == 10 and bq.gp_log_l is not gp_log_l
