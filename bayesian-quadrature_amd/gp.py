"""GP objects with the attribute surface ``bayesian_quadrature.BQ`` uses.

The reference delegates its Gaussian processes to the third-party package
``gaussian_processes==1.0.5`` (import name ``gp``, requirements.txt:2), which is
not in the reference tree.  This module restates the part of its interface
that ``bq.py`` touches (call sites bq.py:147-162,
200,227-228,282-283,325,334-339,465,493-496,546,555-556,936,942-943,953-954)
over the device engine: the Gram matrix, its Cholesky factor, ``K^-1 y``, the
log marginal likelihood and the posterior mean / covariance are computed by
the HIP kernels and memoised until a parameter or the data change.

Formulas: Gaussian kernel ``h^2 N(x1 | x2, w^2)``,
``Kxx = K(x, x) + s^2 I``, ``log_lh = -1/2 y' Kxx^-1 y - 1/2 log|Kxx| - n/2 log 2 pi``.
"""
import copy as _copy

import numpy as np
import scipy.optimize as optim

from . import util
from .engine import get_engine, _marginal_no_mixture, _sq_gaussian_only
from .measures import Measure

DTYPE = np.float64


class GaussianKernel(object):
    """k(x1, x2) = h^2 / (sqrt(2 pi) w) exp(-(x1 - x2)^2 / (2 w^2))."""

    def __init__(self, h, w):
        self.h = None
        self.w = None
        self.set_param("h", h)
        self.set_param("w", w)

    @property
    def params(self):
        return np.array([self.h, self.w], dtype=DTYPE)

    @params.setter
    def params(self, val):
        self.set_param("h", val[0])
        self.set_param("w", val[1])

    def set_param(self, name, val):
        if name not in ("h", "w"):
            raise AttributeError("unknown parameter: %s" % name)
        val = float(val)
        if not np.isfinite(val) or val <= 0:
            raise ValueError("invalid value for %s: %s" % (name, val))
        setattr(self, name, val)

    def copy(self):
        return GaussianKernel(self.h, self.w)

    def __call__(self, x1, x2):
        x1 = np.atleast_1d(np.asarray(x1, dtype=DTYPE))
        x2 = np.atleast_1d(np.asarray(x2, dtype=DTYPE))
        if x1.size == 0 or x2.size == 0:
            return np.empty((x1.size, x2.size), dtype=DTYPE)
        return np.ascontiguousarray(get_engine().gram_cross(x1, x2, self.h, self.w))

    def __getstate__(self):
        return {"h": self.h, "w": self.w}

    def __setstate__(self, state):
        self.h, self.w = state["h"], state["w"]


class PeriodicKernel(object):
    """Placeholder so that ``kernel is PeriodicKernel`` comparisons work
    (bq.py:125); the periodic / approximate branch is outside the MI355X hot
    path and is not implemented."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("PeriodicKernel is out of scope of the MI355X engine")


class GP(object):
    """1-D GP regression y = f(x) + N(0, s^2) over the device engine."""

    def __init__(self, K, x, y, s=0):
        self._memoized = {}
        self._fit = None
        self._fit_params = None
        self.K = K
        self._x = None
        self._y = None
        self._s = None
        self.x = x
        self.y = y
        self.s = s

    # -- memoisation ----------------------------------------------------------
    def _invalidate(self, data_changed=True):
        """Drop every cached quantity.  The device fit object survives a pure
        parameter change: it keeps x and y resident and is re-factored in place
        (bq_gp_refit) on next use -- the hyper-parameter loop's common case."""
        self._memoized = {}
        fit = getattr(self, "_fit", None)
        if fit is not None and data_changed:
            fit.close()
            self._fit = None
        self._fit_params = None

    def _memo(self, key, fn):
        if key not in self._memoized:
            self._memoized[key] = fn()
        return self._memoized[key]

    def _device_fit(self):
        """Gram + Cholesky + z + log-ML on the GPU; raises LinAlgError."""
        params = (self.K.h, self.K.w, self._s)
        if self._fit is None:
            self._fit = get_engine().gp_fit(self._x, self._y, *params)
            self._fit_params = params
        elif self._fit_params != params:
            try:
                self._fit.refit(*params)
            except Exception:
                self._fit_params = None
                raise
            self._fit_params = params
        return self._fit

    # -- data and parameters --------------------------------------------------
    @property
    def x(self):
        return self._x

    @x.setter
    def x(self, val):
        val = np.array(val, dtype=DTYPE, copy=True)
        if val.ndim != 1:
            raise ValueError("x must be one-dimensional")
        if self._x is not None and val.shape == self._x.shape and (val == self._x).all():
            return
        self._invalidate()
        self._x = val

    @property
    def y(self):
        return self._y

    @y.setter
    def y(self, val):
        val = np.array(val, dtype=DTYPE, copy=True)
        if val.ndim != 1:
            raise ValueError("y must be one-dimensional")
        if self._y is not None and val.shape == self._y.shape and (val == self._y).all():
            return
        fit = getattr(self, "_fit", None)
        if (fit is not None and self._y is not None and val.shape == self._y.shape
                and hasattr(fit, "set_y")):
            # same points, new targets (the hyper-parameter loop gives GP2 new targets on every
            # evaluation, bq.py:948-954): the device fit stays and is re-factored on next use
            try:
                fit.set_y(val)
            except (ValueError, RuntimeError, MemoryError):  # the engine's error types
                self._invalidate()
            else:
                self._invalidate(data_changed=False)
        else:
            self._invalidate()
        self._y = val

    def append(self, x, y):
        """Add observations: observably the same as assigning the concatenated ``x`` and ``y``,
        but a device fit whose parameters are current grows in place (engine.Fit.append, O(k n^2)
        on the resident factor) instead of being dropped and rebuilt from nothing -- the
        ``add_observation`` half of the active-sampling loop.  A LinAlgError (the new points make
        Kxx singular) leaves the GP as it was."""
        x = np.atleast_1d(np.array(x, dtype=DTYPE, copy=True))
        y = np.atleast_1d(np.array(y, dtype=DTYPE, copy=True))
        if x.ndim != 1:
            raise ValueError("x must be one-dimensional")
        if y.ndim != 1:
            raise ValueError("y must be one-dimensional")
        if x.shape != y.shape:
            raise ValueError("shape mismatch for x and y")
        if x.size == 0:
            return
        new_x = np.concatenate([self._x, x])
        new_y = np.concatenate([self._y, y])
        fit = getattr(self, "_fit", None)
        params = (self.K.h, self.K.w, self._s)
        if fit is not None and self._fit_params == params and hasattr(fit, "append"):
            try:
                fit.append(x, y)
            except np.linalg.LinAlgError:
                raise  # the fit and the data are what they were
            except (ValueError, RuntimeError, MemoryError):  # the engine's error types
                self._invalidate()
            else:
                self._memoized = {}
        else:
            self._invalidate()
        self._x = new_x
        self._y = new_y

    def remove(self, idx):
        """Drop observations: observably the same as assigning ``np.delete(x, idx)`` and
        ``np.delete(y, idx)``, but a device fit whose parameters are current shrinks in place
        (engine.Fit.remove, O(k n^2) on the resident factor) instead of being dropped and rebuilt
        from nothing -- a sliding window, a retired sample, an outlier.  Indices in [-n, n);
        a ValueError (out of range, a duplicate, every point) leaves the GP as it was."""
        idx = np.atleast_1d(np.asarray(idx))
        if idx.ndim != 1:
            raise ValueError("idx must be one-dimensional")
        if idx.size == 0:
            return
        if idx.dtype.kind not in "iu":
            raise ValueError("idx must hold integers")
        n = self._x.size
        idx = idx.astype(np.int64)
        if ((idx < -n) | (idx >= n)).any():
            raise ValueError("index out of range for %d observations" % n)
        idx = np.where(idx < 0, idx + n, idx)
        if np.unique(idx).size != idx.size:
            raise ValueError("an index is given twice")
        if idx.size >= n:
            raise ValueError("cannot remove every observation")
        new_x = np.delete(self._x, idx)
        new_y = np.delete(self._y, idx)
        fit = getattr(self, "_fit", None)
        params = (self.K.h, self.K.w, self._s)
        if fit is not None and self._fit_params == params and hasattr(fit, "remove"):
            try:
                fit.remove(idx)
            except (ValueError, RuntimeError, MemoryError,  # the engine's error types
                    np.linalg.LinAlgError):
                self._invalidate()
            else:
                self._memoized = {}
        else:
            self._invalidate()
        self._x = new_x
        self._y = new_y

    @property
    def s(self):
        return self._s

    @s.setter
    def s(self, val):
        val = float(val)
        if not np.isfinite(val) or val < 0:
            raise ValueError("invalid value for s: %s" % val)
        if self._s is not None and val == self._s:
            return
        self._invalidate(data_changed=False)
        self._s = val

    @property
    def params(self):
        return np.append(self.K.params, self._s)

    @params.setter
    def params(self, val):
        self.set_param("h", val[0])
        self.set_param("w", val[1])
        self.set_param("s", val[2])

    def get_param(self, name):
        if name == "s":
            return self._s
        return getattr(self.K, name)

    def set_param(self, name, val):
        if name == "s":
            self.s = val
            return
        if float(val) == getattr(self.K, name):
            return
        self.K.set_param(name, val)  # ValueError on invalid values (bq.py:539-543)
        self._invalidate(data_changed=False)

    def copy(self, deep=True):
        new = GP(self.K.copy(), self._x, self._y, s=self._s)
        if hasattr(self, "jitter"):
            new.jitter = self.jitter.copy()
        return new

    # -- fitted quantities ----------------------------------------------------
    @property
    def Kxx(self):
        """K(x, x) + s^2 I; the same array object on repeated access
        (tests/test_bq_c.py:43-49 of the reference rely on that)."""
        return self._memo("Kxx", lambda: np.ascontiguousarray(
            get_engine().gram(self._x, self.K.h, self.K.w, self._s)))

    @property
    def Lxx(self):
        return self._memo("Lxx", lambda: np.ascontiguousarray(self._device_fit().L()))

    @property
    def inv_Kxx_y(self):
        return self._memo("inv_Kxx_y", lambda: self._device_fit().alpha())

    @property
    def log_lh(self):
        return self._memo("log_lh", lambda: self._device_fit().logml)

    @property
    def dloglh_dtheta(self):
        """Gradient of ``log_lh`` in the order of ``params``, [d/dh, d/dw, d/ds], from the
        device fit (bq_gp_logml_grad); memoised like ``log_lh``."""
        return self._memo("dloglh_dtheta", lambda: self._device_fit().logml_grad())

    @property
    def d2loglh_dtheta2(self):
        """Hessian of ``log_lh`` in the order of ``params``, 3 x 3 over [h, w, s], from the
        device fit (bq_gp_logml_hess: analytic, nothing differenced); memoised like
        ``dloglh_dtheta``."""
        return self._memo("d2loglh_dtheta2", lambda: self._device_fit().logml_hess())

    def loo(self):
        """Leave-one-out cross-validation at the current parameters: (mean, var, logpred), the
        predictive mean, variance (of the noisy observation: s^2 included) and log density of
        every y_i from the other n - 1 observations (bq_gp_loo: closed form on the device fit,
        nothing refitted); memoised like ``log_lh``.  ``argmin`` of logpred is the observation
        the model predicts worst -- a candidate for ``remove``."""
        return self._memo("loo_points", lambda: self._loo()[:3])

    def _loo(self):
        return self._memo("loo", lambda: self._device_fit().loo())

    @property
    def log_loo(self):
        """The leave-one-out log predictive density, the sum of ``loo()[2]``; memoised."""
        return self._loo()[3]

    @property
    def dlogloo_dtheta(self):
        """Gradient of ``log_loo`` in the order of ``params``, [d/dh, d/dw, d/ds], from the
        device fit (bq_gp_loo_grad); memoised like ``dloglh_dtheta``."""
        return self._memo("dlogloo_dtheta", lambda: self._device_fit().loo_grad()[1])

    def clusters(self, thresh):
        """The single-linkage groups of ``x`` on the host: the sorted points are split wherever
        the gap to the next one exceeds ``thresh``, and a cluster of more than 64 points is cut
        into runs of at most 64.  Singletons are included: the result, a list of index arrays in
        the order of the sorted points, is a partition ready for ``lgo``."""
        thresh = float(thresh)
        if not thresh >= 0:
            raise ValueError("invalid value for thresh: %s" % thresh)
        order = np.argsort(self._x, kind="stable")
        if order.size == 0:
            return []
        cuts = np.flatnonzero(np.diff(self._x[order]) > thresh) + 1
        out = []
        for c in np.split(order, cuts):
            out.extend(c[i:i + 64] for i in range(0, c.size, 64))
        return out

    @staticmethod
    def _group_key(groups):
        """The groups as a tuple of tuples of ints: what the memo is keyed by."""
        try:
            arrs = [np.asarray(g) for g in groups]
        except TypeError:
            raise ValueError("groups must be a sequence of integer index sequences")
        if any(a.ndim != 1 or (a.size and a.dtype.kind not in "iu") for a in arrs):
            raise ValueError("every group must be a one-dimensional sequence of integers")
        return tuple(tuple(a.tolist()) for a in arrs)

    def _lgo(self, groups):
        key = self._group_key(groups)
        return self._memo(("lgo", key), lambda: self._device_fit().lgo(key))

    def lgo(self, groups):
        """Leave-group-out cross-validation at the current parameters: (mean, var, logpred) with
        whole groups of observations left out at once -- ``groups`` is a sequence of disjoint
        index sequences of 1 to 64 indices each, such as ``clusters(thresh)``; a point in no
        group is never left out.  mean and var follow the concatenated groups, logpred has one
        joint log density per group (bq_gp_lgo: closed form on the device fit, nothing
        refitted).  Memoised per tuple of groups, and dropped by what drops ``loo``.  Where
        samples lie next to each other ``loo`` is flattered by the neighbour that stays in;
        leaving the cluster out is not."""
        return self._lgo(groups)[:3]

    def log_lgo(self, groups):
        """The leave-group-out log predictive density, the sum of ``lgo(groups)[2]``; memoised."""
        return self._lgo(groups)[3]

    def dloglgo_dtheta(self, groups):
        """Gradient of ``log_lgo(groups)`` in the order of ``params``, [d/dh, d/dw, d/ds], from
        the device fit (bq_gp_lgo_grad); memoised like ``lgo``."""
        key = self._group_key(groups)
        return self._memo(("dloglgo_dtheta", key), lambda: self._device_fit().lgo_grad(key)[1])

    def hyper_cov(self, params):
        """Laplace covariance of the named subset of ("h", "w", "s") at the current parameters:
        the inverse of minus the Hessian of ``log_lh`` restricted to them, in their own units
        and their given order.  The other parameters are held fixed, not marginalised.
        numpy.linalg.LinAlgError when that block of -H is not positive definite: the point is not
        a maximum over these parameters (a saddle, a ridge, or an optimum not yet reached)."""
        names = ("h", "w", "s")
        params = list(params)
        if not params or any(p not in names for p in params) or len(set(params)) != len(params):
            raise ValueError("params: a subset of %s" % (names,))
        idx = [names.index(p) for p in params]
        A = -self.d2loglh_dtheta2[np.ix_(idx, idx)]
        if not np.all(np.isfinite(A)):
            raise np.linalg.LinAlgError("the Hessian is not finite")
        np.linalg.cholesky(A)  # LinAlgError unless positive definite
        C = np.linalg.inv(A)
        return 0.5 * (C + C.T)

    def fit_MLII(self, params, method="L-BFGS-B", ntry=10, objective="log_lh", groups=None):
        """Maximise ``log_lh`` over the named subset of ("h", "w", "s") with the exact gradient
        (util.find_good_parameters with ``logpdf_grad``).  ``objective="loo"`` maximises the
        leave-one-out log predictive density ``log_loo`` with ``dlogloo_dtheta`` instead, and
        ``objective="lgo"`` the leave-group-out density ``log_lgo(groups)`` with
        ``dloglgo_dtheta(groups)``: ``groups`` (see ``lgo``) is required for it, fixed for the
        whole optimisation, and must be None for the other objectives.  Any other objective is a
        ValueError.

        Positivity by reparametrisation: the search runs over log h, log w and log s, so every
        point it evaluates has h, w, s > 0 and none lies on the edge s = 0, where Kxx of close
        points is singular.  An optimum at s = 0 is therefore only approached, never reached.
        An s that starts at exactly 0 has no logarithm: it is searched as it is, under the
        L-BFGS-B bound s >= 0.  Leaves the GP at the optimum and returns the optimiser's summary
        (x in the parameters' own units); RuntimeError when no optimum is found."""
        if objective not in ("log_lh", "loo", "lgo"):
            raise ValueError("objective: 'log_lh', 'loo' or 'lgo'")
        if (objective == "lgo") != (groups is not None):
            raise ValueError("groups: required for objective 'lgo', None otherwise")
        if groups is not None:
            groups = self._group_key(groups)
        value = {"log_lh": lambda: self.log_lh, "loo": lambda: self.log_loo,
                 "lgo": lambda: self.log_lgo(groups)}[objective]
        gradient = {"log_lh": lambda: self.dloglh_dtheta, "loo": lambda: self.dlogloo_dtheta,
                    "lgo": lambda: self.dloglgo_dtheta(groups)}[objective]
        names = ("h", "w", "s")
        params = list(params)
        if not params or any(p not in names for p in params) or len(set(params)) != len(params):
            raise ValueError("params: a subset of %s" % (names,))
        idx = [names.index(p) for p in params]
        th0 = np.array([self.get_param(p) for p in params], dtype=DTYPE)
        logp = th0 > 0
        u0 = np.where(logp, np.log(np.where(logp, th0, 1.0)), th0)
        bounds = [(None, None) if lg else (0.0, None) for lg in logp]

        def theta(u):
            return np.where(logp, np.exp(u), u)

        def set_all(t):
            for p, v in zip(params, t):
                self.set_param(p, v)

        def logpdf(u):
            try:
                set_all(theta(u))
                return value()
            except (ValueError, np.linalg.LinAlgError):
                return -np.inf

        def logpdf_grad(u):
            f = logpdf(u)
            if not np.isfinite(f):
                return f, np.zeros(len(params))
            t = theta(u)
            g = gradient()
            return f, g[idx] * np.where(logp, t, 1.0)

        u = util.find_good_parameters(logpdf, u0, method, ntry=ntry, logpdf_grad=logpdf_grad,
                                      bounds=bounds if method == "L-BFGS-B" else None)
        if u is None:
            set_all(th0)
            raise RuntimeError("couldn't find good parameters")
        x = theta(u)
        set_all(x)
        opt = util.LAST_OPT
        fun = -value()
        return optim.OptimizeResult(x=x, fun=fun, success=opt.get("success", False),
                                    nfev=opt.get("nfev", -1), nit=opt.get("nit", -1),
                                    attempts=opt.get("attempts", -1))

    def Kxoxo(self, xo):
        return self.K(xo, xo)

    def Kxxo(self, xo):
        return self.K(self._x, xo)

    def Kxox(self, xo):
        return self.K(xo, self._x)

    def mean(self, xo):
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            return np.empty(0, dtype=DTYPE)
        return self._device_fit().predict(xo, want_mean=True, want_var=False)[0]

    def var(self, xo):
        """diag(cov(xo)) without forming the M x M matrix (what bq.py:227 and
        :943 need)."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            return np.empty(0, dtype=DTYPE)
        return self._device_fit().predict(xo, want_mean=False, want_var=True)[1]

    def mean_var(self, xo):
        """Posterior mean and marginal variance.  When new hyper-parameters are still waiting
        for their refit -- the hyper-parameter loop (bq.py:933-947) sets them and asks for the
        candidates' posterior next -- both happen in one device sweep."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        params = (self.K.h, self.K.w, self._s)
        fit = self._fit
        if (fit is not None and self._fit_params != params and 0 < xo.size <= 63
                and hasattr(fit, "refit_predict")):
            try:
                m, v = fit.refit_predict(*params, xo)
            except Exception:
                self._fit_params = None
                raise
            self._fit_params = params
            return m, v
        m, v, _ = self._device_fit().predict(xo, want_mean=True, want_var=True)
        return m, v

    @staticmethod
    def _grad_shape(xo, g):
        """A gradient as the device returns it, (d, M), in the shape of the points it was asked at:
        (M,) for a vector of points."""
        return g[0] if xo.ndim == 1 else g

    def dmean_dx(self, xo):
        """Gradient of ``mean`` with respect to the points: entry [j] (or [k, j] for d x M points)
        is d mean(xo_j) / d xo_j, in closed form on the device fit (bq_gp_predict_grad, the route
        without a sweep)."""
        return self._mean_grad(xo)[1]

    def _mean_grad(self, xo):
        """(mean, dmean_dx) from the one fused launch."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            return np.empty(0, dtype=DTYPE), np.empty(xo.shape, dtype=DTYPE)
        m, _, dm, _ = self._device_fit().predict_grad(xo, want_var=False)
        return m, self._grad_shape(xo, dm)

    def dvar_dx(self, xo):
        """Gradient of ``var`` with respect to the points, shaped like ``dmean_dx``'s."""
        return self.mean_var_grad(xo)[3]

    def mean_var_grad(self, xo):
        """(mean, var, dmean_dx, dvar_dx) at the points in one device call: the prediction's
        sweep, one backward sweep and one reduction more (bq_gp_predict_grad)."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            e = np.empty(0, dtype=DTYPE)
            return e, e.copy(), np.empty(xo.shape, dtype=DTYPE), np.empty(xo.shape, dtype=DTYPE)
        m, v, dm, dv = self._device_fit().predict_grad(xo, want_var=True)
        return m, v, self._grad_shape(xo, dm), self._grad_shape(xo, dv)

    def dmean_dtheta(self, xo):
        """Derivatives of ``mean`` with respect to the hyper-parameters, (3, M) in the order of
        ``params``: row p is d mean(xo_j) / d [h, w, s][p], in closed form on the device fit
        (bq_gp_predict_dtheta, the route without a sweep)."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            return np.empty((3, 0), dtype=DTYPE)
        return self._device_fit().predict_dtheta(xo, want_var=False)[2]

    def dvar_dtheta(self, xo):
        """Derivatives of ``var`` with respect to the hyper-parameters, shaped like
        ``dmean_dtheta``'s."""
        return self.mean_var_dtheta(xo)[3]

    def mean_var_dtheta(self, xo):
        """(mean, var, dmean_dtheta, dvar_dtheta) at the points in one device call: the
        prediction's sweep, one backward sweep, one product per length scale and one reduction
        (bq_gp_predict_dtheta)."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            e = np.empty(0, dtype=DTYPE)
            return e, e.copy(), np.empty((3, 0), dtype=DTYPE), np.empty((3, 0), dtype=DTYPE)
        return self._device_fit().predict_dtheta(xo, want_var=True)

    def mean_var_laplace(self, xo, params):
        """(mean, var + g^T C g): the predictive variance with the named subset of
        ("h", "w", "s") marginalised to first order around the current parameters -- g the rows
        of ``dmean_dtheta`` for that subset, C = ``hyper_cov(params)``, the Laplace covariance of
        an ML-II optimum.  Raises what ``hyper_cov`` raises: ValueError for bad names,
        numpy.linalg.LinAlgError away from a maximum."""
        Cov = self.hyper_cov(params)
        idx = [("h", "w", "s").index(p) for p in params]
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            e = np.empty(0, dtype=DTYPE)
            return e, e.copy()
        # (the prediction, then the mean's derivatives on the route without a sweep: dvar's
        # product per length scale is not needed here)
        fit = self._device_fit()
        m, v, _ = fit.predict(xo, want_mean=True, want_var=True)
        g = fit.predict_dtheta(xo, want_var=False)[2][idx]
        return m, v + np.einsum("pj,pq,qj->j", g, Cov, g)

    # -- the polynomial trend, its coefficients marginalised -------------------
    @staticmethod
    def _trend_degree(degree):
        if isinstance(degree, bool) or degree not in (0, 1, 2):
            raise ValueError("invalid value for degree: %s" % (degree,))
        return int(degree)

    def _trend_basis(self):
        """(center, scale) of the trend's basis: the mean of ``x`` and the largest ``|x - center|``
        (1 where that is 0), so that the scaled points fill [-1, 1]; memoised with the data."""
        def make():
            c = float(np.mean(self._x))
            r = float(np.max(np.abs(self._x - c)))
            return np.array([c], dtype=DTYPE), np.array([r if r > 0 else 1.0], dtype=DTYPE)
        return self._memo("trend_basis", make)

    def trend(self, degree=2):
        """(beta, cov_beta, logml_t, alpha_t): a polynomial trend of ``degree`` 0, 1 or 2 under the
        GP, ``y = phi(x)^T beta + f(x) + noise`` with a flat prior on beta that is integrated out
        (universal kriging; engine.Fit.trend, bq_gp_trend).  phi is [1, t, t^2][:degree + 1] in
        ``t = (x - center) / scale`` with ``_trend_basis``'s centre and scale.  beta: the
        coefficients' posterior mean; cov_beta: their covariance; logml_t: ``log_lh_trend``;
        alpha_t: ``Kxx^-1 (y - H beta)``.  A view of the fit, memoised like ``log_lh``:
        ``mean``, ``var``, ``log_lh`` and everything else stay those of the zero-mean GP."""
        degree = self._trend_degree(degree)
        return self._memo(("trend", degree),
                          lambda: self._device_fit().trend(degree, *self._trend_basis()))

    def log_lh_trend(self, degree=2):
        """The log marginal likelihood with the trend's coefficients integrated out (Rasmussen &
        Williams 2.45).  The flat prior leaves its additive constant to the basis: values compare
        across hyper-parameters of one data set, not across degrees or rescaled data."""
        return self.trend(degree)[2]

    def mean_trend(self, xo, degree=2):
        """Posterior mean under the trend (bq_gp_predict_trend, the route without a sweep): away
        from the data it follows the fitted polynomial where ``mean`` goes back to 0."""
        degree = self._trend_degree(degree)
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            return np.empty(0, dtype=DTYPE)
        return self._device_fit().predict_trend(xo, degree, *self._trend_basis(),
                                                want_var=False)[0]

    def var_trend(self, xo, degree=2):
        """Posterior variance under the trend: ``var`` plus the uncertainty of the coefficients."""
        return self.mean_var_trend(xo, degree)[1]

    def mean_var_trend(self, xo, degree=2):
        """(mean_trend, var_trend) at the points in one device call: the prediction's sweep with
        the trend's sums in its row reductions (bq_gp_predict_trend)."""
        degree = self._trend_degree(degree)
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            e = np.empty(0, dtype=DTYPE)
            return e, e.copy()
        return self._device_fit().predict_trend(xo, degree, *self._trend_basis(), want_var=True)

    def cov(self, xo):
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        if xo.size == 0:
            return np.empty((0, 0), dtype=DTYPE)
        c = self._device_fit().predict(xo, want_mean=False, want_var=True, want_cov=True)[2]
        return np.ascontiguousarray(c)

    def sample(self, xo, n=1, seed=None, z=None, ladder=None, return_info=False):
        """``n`` joint draws of the latent function at the points, (n, M): row i is
        ``mean(xo) + L_c z_i`` with ``L_c L_c^T = cov(xo) + jitter I`` (no s^2, as ``cov``), all on
        the device fit (bq_gp_sample) -- sample paths, Thompson draws over a candidate grid,
        Monte-Carlo propagation of the posterior.  ``xo`` is a vector of points, or d x M as for
        ``dmean_dx``.  A smooth posterior at dense points is numerically singular, so the jitter
        is part of the contract: k(x, x) times the first entry of ``ladder`` (default 0, 1e-12,
        1e-10, 1e-8, 1e-6) at which the covariance factors; numpy.linalg.LinAlgError when none
        does.  ``z``: (n, M) standard normals to use; None: the device draws them from ``seed``,
        and ``seed=None`` takes a 64-bit seed from ``numpy.random``, so ``np.random.seed`` makes a
        script reproducible.  ``return_info`` appends {"mean", "jitter"}."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        n = int(n)
        if n < 1:
            raise ValueError("invalid value for n: %s" % n)
        M = xo.shape[-1] if xo.ndim <= 2 else -1
        if z is not None:
            z = np.asarray(z, dtype=DTYPE)
            if z.shape != (n, M):
                raise ValueError("z must be (n, M)")
        if xo.size == 0:
            out = np.empty((n, 0), dtype=DTYPE)
            info = {"mean": np.empty(0, dtype=DTYPE), "jitter": 0.0}
            return (out, info) if return_info else out
        if z is None and seed is None:
            seed = int(np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64)
                       .dot(np.array([1, 2 ** 32], dtype=np.uint64)))
        out, mean, jitter = self._device_fit().sample(
            xo, S=n, z=None if z is None else z.T, seed=0 if seed is None else seed,
            ladder=ladder)
        out = np.ascontiguousarray(out.T)
        return (out, {"mean": mean, "jitter": jitter}) if return_info else out

    def pivoted_cholesky(self, xo, q, noisy=False, tol=0.0):
        """(piv, C, resid, gain): the greedy, diagonally pivoted partial Cholesky factorisation of
        ``cov(xo)`` in at most ``q`` steps, on the device fit and without forming the covariance
        (bq_gp_pivchol) -- a candidate grid far too large for ``cov`` is fine.  Each step takes the
        point whose remaining variance is largest.  piv: the chosen indices into ``xo``, (rank,);
        C: (M, rank) Fortran-ordered, the best greedy rank-``rank`` factor, ``C C^T ~ cov(xo)``;
        resid: (M,), the variance left at every point, ``diag(cov - C C^T)``; gain: (rank,), the
        variance each pivot had when it was taken.  ``noisy`` puts the nugget s^2 under the square
        root: resid is then the posterior variance after noisy observations at the pivots, a
        point may be taken twice, and nothing is zeroed; without it a taken point keeps resid 0.
        rank < q when a gain falls to ``tol`` k(x, x) or is not positive.  ``xo`` is a vector of
        points, or d x M as for ``dmean_dx``."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        q = int(q)
        if q < 1:
            raise ValueError("invalid value for q: %s" % q)
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError("invalid value for tol: %s" % tol)
        if xo.size == 0:
            return (np.empty(0, dtype=np.int64), np.empty((0, 0), dtype=DTYPE, order="F"),
                    np.empty(0, dtype=DTYPE), np.empty(0, dtype=DTYPE))
        M = xo.shape[-1]
        if q > M:
            raise ValueError("q = %d steps over %d points" % (q, M))
        return self._device_fit().pivoted_cholesky(
            xo, q, nugget=float(self._s) ** 2 if noisy else 0.0, tol=float(tol))

    def greedy_design(self, xo, q, noisy=True, tol=0.0, return_info=False):
        """The indices into ``xo`` of a batch of at most ``q`` points to evaluate next: the
        max-variance sequential design, each point chosen where the variance is largest once the
        points before it count as observed -- ``pivoted_cholesky``'s pivots; unlike the ``q``
        largest marginal variances they do not crowd one peak.  ``noisy`` (the default) counts an
        observation with the noise s^2, as ``append`` would.  ``return_info`` appends {"gain",
        "resid"}: the variance each chosen point had, and the variance left everywhere."""
        piv, _, resid, gain = self.pivoted_cholesky(xo, q, noisy=noisy, tol=tol)
        return (piv, {"gain": gain, "resid": resid}) if return_info else piv

    def _ivr(self, xo, q, ref, weights, noisy, tol, want_scores):
        """The checked arguments of ``ivr_design`` / ``ivr_scores`` and the device call; None for
        empty ``xo``."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        q = int(q)
        if q < 1:
            raise ValueError("invalid value for q: %s" % q)
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError("invalid value for tol: %s" % tol)
        if xo.ndim > 2 or (ref is not None and np.ndim(ref) > 2):
            raise ValueError("points must be a vector or a d x M matrix")
        if xo.size == 0:
            return None
        if q > xo.shape[-1]:
            raise ValueError("q = %d steps over %d points" % (q, xo.shape[-1]))
        d = 1 if xo.ndim == 1 else xo.shape[0]
        if ref is not None:
            ref = np.atleast_1d(np.asarray(ref, dtype=DTYPE))
            if ref.size == 0:
                raise ValueError("no reference points")
            if (1 if ref.ndim == 1 else ref.shape[0]) != d:
                raise ValueError("dimension mismatch")
        R = (xo if ref is None else ref).shape[-1]
        if weights is not None:
            weights = np.atleast_1d(np.asarray(weights, dtype=DTYPE))
            if weights.shape != (R,):
                raise ValueError("%s weights for %d reference points" % (weights.shape, R))
            if not (np.all(np.isfinite(weights)) and np.all(weights >= 0)):
                raise ValueError("weights must be finite and not negative")
        return self._device_fit().ivr_design(
            xo, q, xr=ref, rho=weights, nugget=float(self._s) ** 2 if noisy else 0.0,
            tol=float(tol), want_scores=want_scores)

    def ivr_design(self, xo, q, ref=None, weights=None, noisy=True, tol=0.0, return_info=False):
        """The indices into ``xo`` of a batch of at most ``q`` points to evaluate next, chosen to
        lower the integrated posterior variance ``sum_j weights_j var(ref_j)`` the most, one point
        at a time with the points before it counted as observed (integrated variance reduction;
        ALC, IMSPE) -- on the device fit (bq_gp_ivr).  ``greedy_design`` asks where the model is
        least sure, which is the edge of the candidate box; this asks which observation teaches
        the most about the region that ``ref`` and ``weights`` describe: a grid or a sample of the
        measure one integrates against.  ``ref`` None: the candidates themselves; ``weights``
        None: uniform.  ``noisy`` (the default) counts an observation with the noise s^2, as
        ``append`` would, and a point may then be chosen twice.  Fewer than ``q`` indices come
        back when a step's gain falls to ``tol`` k(x, x) sum(weights) or is not positive.
        ``return_info`` appends {"gain": the drop each step brought, "ivar0": the integral before,
        "resid": the variance left at ``xo``, "resid_ref": at ``ref``}.  ``xo`` and ``ref`` are
        vectors of points, or d x M as for ``pivoted_cholesky``."""
        out = self._ivr(xo, q, ref, weights, noisy, tol, False)
        if out is None:
            piv, gain, ivar0 = np.empty(0, dtype=np.int64), np.empty(0, dtype=DTYPE), 0.0
            resid_r = resid_c = np.empty(0, dtype=DTYPE)
        else:
            piv, gain, ivar0, resid_r, resid_c = out
        info = {"gain": gain, "ivar0": ivar0, "resid": resid_c, "resid_ref": resid_r}
        return (piv, info) if return_info else piv

    def ivr_scores(self, xo, ref=None, weights=None, noisy=True):
        """(M,): how much observing each point of ``xo`` alone would lower the integrated
        posterior variance ``sum_j weights_j var(ref_j)`` -- the acquisition surface that
        ``ivr_design``'s first step takes the maximum of (arguments as there)."""
        out = self._ivr(xo, 1, ref, weights, noisy, 0.0, True)
        return np.empty(0, dtype=DTYPE) if out is None else out[5]

    def _measure(self, mu, cov):
        """(mu, cov, key): the measure of an integral, checked, and its memoisation key.  A
        Gaussian is a (d,) vector and a (d, d) matrix; a ``measures.BoxMeasure`` or
        ``measures.GaussianMixture`` in place of mu, with no cov, comes back as (measure, None)."""
        d = 1 if self._x.ndim == 1 else self._x.shape[0]
        if isinstance(mu, Measure):
            if cov is not None:
                raise TypeError("a measure object comes without a cov")
            if mu.d != d:
                raise ValueError("the measure has dimension %d, the GP %d" % (mu.d, d))
            return mu, None, mu.key
        if cov is None:
            raise TypeError("a Gaussian measure needs its cov")
        mu = np.ascontiguousarray(np.atleast_1d(mu), dtype=DTYPE)
        cov = np.ascontiguousarray(np.atleast_2d(cov), dtype=DTYPE)
        if mu.shape != (d,):
            raise ValueError("mu has invalid shape")
        if cov.shape != (d, d):
            raise ValueError("cov has invalid shape")
        if not (np.all(np.isfinite(mu)) and np.all(np.isfinite(cov))):
            raise ValueError("the measure must be finite")
        return mu, cov, (mu.tobytes(), cov.tobytes())

    @staticmethod
    def _margs(mu, cov):
        """The measure as the positional arguments of the fit's calls: (mu, cov) for a Gaussian,
        (measure,) for an object."""
        return (mu,) if cov is None else (mu, cov)

    def _integral(self, mu, cov):
        mu, cov, key = self._measure(mu, cov)
        return self._memo(("integral", key),
                          lambda: self._device_fit().integral(*self._margs(mu, cov),
                                                              want_weights=True))

    def integral(self, mu, cov=None):
        """(mean, var): vanilla Bayesian quadrature of the GP, the posterior mean and variance of
        ``Z = int f(x) N(x | mu, cov) dx`` (engine.Fit.integral, bq_gp_integral): for the Gaussian
        kernel and a Gaussian measure every ingredient is closed form.  So it is for the uniform
        measure on a box and for a mixture of Gaussians: a ``measures.BoxMeasure`` or
        ``measures.GaussianMixture`` in place of ``mu``, with no ``cov``, integrates against that
        (here and in ``integral_weights``, ``integral_design`` and ``integral_scores``).  ``var``
        is latent, like ``var(xo)`` without s^2.  A view of the fit, memoised per measure like
        ``log_lh``."""
        return self._integral(mu, cov)[:2]

    def integral_weights(self, mu, cov=None):
        """(n,): the quadrature weights ``Kxx^-1 kappa_X`` of ``integral``, whose mean is
        ``integral_weights . y``."""
        return self._integral(mu, cov)[2].copy()

    def _marginal(self, axes, xo, mu, cov, want_cov):
        _marginal_no_mixture(mu)
        mu, cov, key = self._measure(mu, cov)
        axes = tuple(int(a) for a in np.atleast_1d(np.asarray(axes)).ravel())
        xo = np.ascontiguousarray(xo, dtype=DTYPE)
        mkey = ("marginal", want_cov, axes, xo.shape, xo.tobytes(), key)
        return self._memo(mkey, lambda: self._device_fit().marginal(
            xo, axes, *self._margs(mu, cov), want_mean=not want_cov, want_var=not want_cov,
            want_cov=want_cov))

    def marginal(self, axes, xo, mu, cov=None):
        """(mean, var), (M,) each: the marginal of the GP over every axis but ``axes``,
        ``J(q) = int f(q, t) pi(q, t) dt`` at the points ``xo`` -- (|S|, M), or (M,) for one kept
        axis -- under the Gaussian ``(mu, cov)`` or a ``measures.BoxMeasure`` on all d axes
        (engine.Fit.marginal, bq_gp_marginal).  J is unnormalised: it integrates to
        ``integral``'s mean, and ``J / Z`` is the marginal posterior density.  ``var`` is latent.
        A GP over fewer than two axes has no marginal (ValueError); neither has a
        ``measures.GaussianMixture``.  A view of the fit, memoised like ``integral``."""
        mean, var, _ = self._marginal(axes, xo, mu, cov, False)
        return mean.copy(), var.copy()

    def marginal_cov(self, axes, xo, mu, cov=None):
        """(M, M): the joint covariance of ``marginal`` at the points ``xo``; its double integral
        over q is ``integral``'s var."""
        return self._marginal(axes, xo, mu, cov, True)[2].copy()

    def _zdesign(self, xo, q, mu, cov, noisy, tol, want_scores):
        """The checked arguments of ``integral_design`` / ``integral_scores`` and the device
        call; None for empty ``xo``."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        q = int(q)
        if q < 1:
            raise ValueError("invalid value for q: %s" % q)
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError("invalid value for tol: %s" % tol)
        if xo.ndim > 2:
            raise ValueError("points must be a vector or a d x M matrix")
        mu, cov, _ = self._measure(mu, cov)
        if xo.size == 0:
            return None
        if q > xo.shape[-1]:
            raise ValueError("q = %d steps over %d points" % (q, xo.shape[-1]))
        return self._device_fit().integral_design(
            xo, q, *self._margs(mu, cov), nugget=float(self._s) ** 2 if noisy else 0.0, tol=float(tol),
            want_scores=want_scores)

    def integral_design(self, xo, q, mu, cov=None, noisy=True, tol=0.0, return_info=False):
        """The indices into ``xo`` of a batch of at most ``q`` points to evaluate next, chosen to
        lower the posterior variance of ``Z = int f(x) N(x | mu, cov) dx`` the most, one point at
        a time with the points before it counted as observed (sequential Bayesian quadrature) --
        on the device fit (bq_gp_zdesign).  ``ivr_design`` lowers the variance of the function
        averaged over reference points that stand for the measure; this lowers the variance of
        the integral itself and needs no reference points.  ``noisy`` (the default) counts an
        observation with the noise s^2, as ``append`` would, and a point may then be chosen
        twice.  Fewer than ``q`` indices come back when a step's gain falls to ``tol`` times the
        prior variance of Z or is not positive.  ``return_info`` appends {"gain": the drop of
        var Z each step brought, "zvar0": ``integral``'s var before, "resid": the variance left
        at ``xo``, "resid_u": the covariance of Z with the function at ``xo`` that is left}.
        ``xo`` is a vector of points, or d x M as for ``pivoted_cholesky``."""
        out = self._zdesign(xo, q, mu, cov, noisy, tol, False)
        if out is None:
            piv, gain = np.empty(0, dtype=np.int64), np.empty(0, dtype=DTYPE)
            zvar0 = self.integral(mu, cov)[1]
            resid_u = resid_c = np.empty(0, dtype=DTYPE)
        else:
            piv, gain, zvar0, resid_u, resid_c = out
        info = {"gain": gain, "zvar0": zvar0, "resid": resid_c, "resid_u": resid_u}
        return (piv, info) if return_info else piv

    def integral_scores(self, xo, mu, cov=None, noisy=True):
        """(M,): how much observing each point of ``xo`` alone would lower the posterior variance
        of ``Z = int f(x) N(x | mu, cov) dx`` -- the acquisition surface that
        ``integral_design``'s first step takes the maximum of (arguments as there)."""
        out = self._zdesign(xo, 1, mu, cov, noisy, 0.0, True)
        return np.empty(0, dtype=DTYPE) if out is None else out[5]

    def sq_integral(self, mu, cov):
        """(sq, var): square-root-warped Bayesian quadrature of the GP (WSABI-L; engine.Fit.
        sq_integral, bq_gp_sqintegral).  With the GP's targets g = sqrt(2 (l - alpha0)) of an
        integrand l >= alpha0 and l = alpha0 + g^2 / 2 linearised about the posterior mean m,
        ``sq = int m(x)^2 N(x | mu, cov) dx`` -- the integral of l has mean alpha0 + sq / 2 -- and
        ``var`` is its variance, latent like ``integral``'s.  ``wsabi.SqrtBQ`` keeps alpha0.  A view
        of the fit, memoised like ``integral``."""
        _sq_gaussian_only(mu)
        mu, cov, key = self._measure(mu, cov)
        return self._memo(("sq_integral", key), lambda: self._device_fit().sq_integral(mu, cov))

    def _sqdesign(self, xo, q, mu, cov, noisy, tol, want_scores):
        """``_zdesign`` for the warped integral."""
        xo = np.atleast_1d(np.asarray(xo, dtype=DTYPE))
        q = int(q)
        if q < 1:
            raise ValueError("invalid value for q: %s" % q)
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError("invalid value for tol: %s" % tol)
        if xo.ndim > 2:
            raise ValueError("points must be a vector or a d x M matrix")
        _sq_gaussian_only(mu)
        mu, cov, _ = self._measure(mu, cov)
        if xo.size == 0:
            return None
        if q > xo.shape[-1]:
            raise ValueError("q = %d steps over %d points" % (q, xo.shape[-1]))
        return self._device_fit().sq_integral_design(
            xo, q, mu, cov, nugget=float(self._s) ** 2 if noisy else 0.0, tol=float(tol),
            want_scores=want_scores)

    def sq_integral_design(self, xo, q, mu, cov, noisy=True, tol=0.0, return_info=False):
        """``integral_design`` for the square-root-warped integral of ``sq_integral``: the indices
        into ``xo`` of at most ``q`` points whose observation lowers the variance of the
        linearised integral the most, one at a time, with the posterior mean about which the
        integrand is linearised held at its current value (bq_gp_sqdesign).  ``tol`` is in
        multiples of the prior variance of that integral; ``return_info`` appends {"gain",
        "zvar0": ``sq_integral``'s var before, "resid", "resid_u"} as ``integral_design`` does."""
        out = self._sqdesign(xo, q, mu, cov, noisy, tol, False)
        if out is None:
            piv, gain = np.empty(0, dtype=np.int64), np.empty(0, dtype=DTYPE)
            zvar0 = self.sq_integral(mu, cov)[1]
            resid_u = resid_c = np.empty(0, dtype=DTYPE)
        else:
            piv, gain, zvar0, resid_u, resid_c = out
        info = {"gain": gain, "zvar0": zvar0, "resid": resid_c, "resid_u": resid_u}
        return (piv, info) if return_info else piv

    def sq_integral_scores(self, xo, mu, cov, noisy=True):
        """(M,): how much observing each point of ``xo`` alone would lower the variance of the
        square-root-warped integral -- step 0's surface of ``sq_integral_design``."""
        out = self._sqdesign(xo, 1, mu, cov, noisy, 0.0, True)
        return np.empty(0, dtype=DTYPE) if out is None else out[5]

    # -- pickling / copying: only data and parameters travel -------------------
    def __getstate__(self):
        state = {"K": self.K, "x": self._x, "y": self._y, "s": self._s}
        if hasattr(self, "jitter"):
            state["jitter"] = self.jitter
        return state

    def __setstate__(self, state):
        self._memoized = {}
        self._fit = None
        self._fit_params = None
        self.K = state["K"]
        self._x, self._y, self._s = state["x"], state["y"], state["s"]
        if "jitter" in state:
            self.jitter = state["jitter"]

    def __copy__(self):
        new = GP.__new__(GP)
        new.__setstate__(self.__getstate__())
        return new

    def __deepcopy__(self, memo):
        new = GP.__new__(GP)
        new.__setstate__(_copy.deepcopy(self.__getstate__(), memo))
        return new

    def __del__(self):
        try:
            if self._fit is not None:
                self._fit.close()
        except Exception:
            pass
