"""CPU tests of the host plumbing of removed observations: gp.GP.remove over a stub engine whose
fit records its calls (its ``remove`` refits the ``np.delete``'d data: numpy stands in for the
device), and over a fit without ``remove`` (the drop-and-refit route)."""
import numpy as np
import pytest

from engine_double import EngineDouble, FitDouble


class RecordingFit(FitDouble):
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
        self.x = np.concatenate([np.ravel(self.x), np.ravel(x_new)])
        self.y = np.concatenate([self.y, np.ravel(y_new)])
        self.n = self.y.shape[0]
        self._L, self._alpha, self.logml = self.o.gp_fit(self.x, self.y, self.h, self.w, self.s)

    def remove(self, idx):
        self.log.append(("remove", tuple(int(i) for i in idx)))
        if self.fail_with is not None:
            raise self.fail_with
        self.x = np.delete(np.ravel(self.x), idx)
        self.y = np.delete(self.y, idx)
        self.n = self.y.shape[0]
        self._L, self._alpha, self.logml = self.o.gp_fit(self.x, self.y, self.h, self.w, self.s)

    def logml_grad(self):
        self.log.append(("grad", self.n))
        return np.zeros(3)

    def close(self):
        self.log.append(("close", self.n))


class NoRemoveFit(RecordingFit):
    remove = property()  # hasattr(fit, "remove") is False


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


IDX = [3, 17, 0, 29]


def test_remove_shrinks_the_fit_once_and_keeps_it(stub, oracle):
    x, y = _data()
    g = _gp(x, y)
    g.log_lh
    fit = g._fit
    g.remove(IDX)
    assert g._fit is fit and _calls(stub, "remove") == [("remove", tuple(IDX))]
    assert not _calls(stub, "close") and len(_calls(stub, "fit")) == 1
    x2, y2 = np.delete(x, IDX), np.delete(y, IDX)
    assert np.array_equal(g.x, x2) and np.array_equal(g.y, y2)
    L, a, lm = oracle.gp_fit(x2, y2, 1.2, 0.8, 0.1)
    assert g.log_lh == lm and np.array_equal(g.Lxx, L) and np.array_equal(g.inv_Kxx_y, a)
    assert len(_calls(stub, "fit")) == 1 and len(_calls(stub, "refit")) == 1  # (the fit's own)
    g.remove(5)  # a scalar index
    assert g._fit is fit and g.x.shape == (25,) and _calls(stub, "remove")[-1] == ("remove", (5,))
    assert np.array_equal(g.x, np.delete(x2, 5))


def test_remove_clears_the_memo(stub):
    x, y = _data()
    g = _gp(x, y)
    L0, lm0, g0 = g.Lxx, g.log_lh, g.dloglh_dtheta
    assert g.Lxx is L0 and len(_calls(stub, "grad")) == 1
    g.remove(IDX)
    assert g._memoized == {}
    assert g.Lxx.shape == (26, 26) and g.log_lh != lm0
    g.dloglh_dtheta
    assert _calls(stub, "grad") == [("grad", 30), ("grad", 26)]


def test_remove_without_a_fit_does_not_touch_the_engine(stub):
    x, y = _data()
    g = _gp(x, y)
    g.remove(IDX)  # never fitted
    assert g._fit is None and not stub.log
    assert np.array_equal(g.x, np.delete(x, IDX)) and np.array_equal(g.y, np.delete(y, IDX))
    g.log_lh
    assert stub.log[0] == ("fit", 26) and not _calls(stub, "remove")


def test_remove_with_pending_parameters_drops_the_fit(stub, oracle):
    x, y = _data()
    g = _gp(x, y)
    g.log_lh
    g.set_param("w", 0.5)  # pending: the resident factor belongs to w = 0.8
    g.remove(IDX)
    assert g._fit is None and _calls(stub, "close") == [("close", 30)]
    assert not _calls(stub, "remove")
    assert g.log_lh == oracle.gp_fit(np.delete(x, IDX), np.delete(y, IDX), 1.2, 0.5, 0.1)[2]
    assert _calls(stub, "fit") == [("fit", 30), ("fit", 26)]


def test_remove_on_a_fit_without_remove_drops_it(stub, oracle):
    stub.fit_class = NoRemoveFit
    x, y = _data()
    g = _gp(x, y)
    g.log_lh
    assert not hasattr(g._fit, "remove")
    g.remove(IDX)
    assert g._fit is None and _calls(stub, "close") == [("close", 30)]
    assert g.log_lh == oracle.gp_fit(np.delete(x, IDX), np.delete(y, IDX), 1.2, 0.8, 0.1)[2]


def test_the_engine_double_takes_the_old_route(oracle, stub):
    """tests/engine_double.py's fit has no ``remove``: the ``hasattr`` guard drops it."""
    from bayesian_quadrature_amd import engine as eng_mod
    eng_mod.set_engine(EngineDouble(oracle), 0)
    x, y = _data()
    g = _gp(x, y)
    g.log_lh
    assert not hasattr(g._fit, "remove")
    g.remove(IDX)
    assert g._fit is None
    assert g.log_lh == oracle.gp_fit(np.delete(x, IDX), np.delete(y, IDX), 1.2, 0.8, 0.1)[2]


@pytest.mark.parametrize("idx", [[30], [-31], [3, 3], [3, -27], list(range(30)), [[1, 2]], [1.5],
                                 [0, 100]])
def test_value_errors_leave_the_gp_as_it_was(stub, idx):
    x, y = _data()
    g = _gp(x, y)
    L0, lm0 = g.Lxx, g.log_lh
    fit = g._fit
    with pytest.raises(ValueError):
        g.remove(idx)
    assert g._fit is fit and np.array_equal(g.x, x) and np.array_equal(g.y, y)
    assert g.Lxx is L0 and g.log_lh == lm0
    assert not _calls(stub, "close") and not _calls(stub, "remove")


def test_negative_indices_count_from_the_end(stub):
    x, y = _data()
    g = _gp(x, y)
    g.log_lh
    g.remove([-1, 2, -30])
    assert _calls(stub, "remove") == [("remove", (29, 2, 0))]
    assert np.array_equal(g.x, np.delete(x, [29, 2, 0]))
    assert np.array_equal(g.y, np.delete(y, [-1, 2, -30]))


def test_an_empty_index_list_is_a_no_op(stub):
    x, y = _data()
    g = _gp(x, y)
    L0 = g.Lxx
    g.remove([])
    g.remove(np.empty(0, dtype=int))
    assert g.Lxx is L0 and g.x.shape == (30,)
    assert not _calls(stub, "remove") and not _calls(stub, "close")


def test_an_engine_error_drops_the_fit_and_still_shrinks_the_data(stub):
    x, y = _data()
    g = _gp(x, y)
    g.log_lh
    g._fit.fail_with = RuntimeError("device lost")
    g.remove(IDX)
    assert g._fit is None and _calls(stub, "close") == [("close", 30)]
    assert np.array_equal(g.x, np.delete(x, IDX)) and np.array_equal(g.y, np.delete(y, IDX))
    g.log_lh
    assert _calls(stub, "fit") == [("fit", 30), ("fit", 26)]


def test_remove_then_append_equals_a_gp_on_the_permuted_data(stub, oracle):
    x, y = _data()
    g = _gp(x, y)
    g.log_lh
    fit = g._fit
    g.remove(IDX)
    g.append(x[IDX], y[IDX])
    assert g._fit is fit and len(_calls(stub, "fit")) == 1
    xp = np.concatenate([np.delete(x, IDX), x[IDX]])
    yp = np.concatenate([np.delete(y, IDX), y[IDX]])
    ref = _gp(xp, yp)
    assert np.array_equal(g.x, ref.x) and np.array_equal(g.y, ref.y)
    assert g.log_lh == ref.log_lh and np.array_equal(g.Lxx, ref.Lxx)
    assert np.array_equal(g.inv_Kxx_y, ref.inv_Kxx_y)
    xo = np.linspace(-3, 3, 7)
    assert np.array_equal(g.mean(xo), ref.mean(xo))
