"""Measures to integrate a fit against, besides the single Gaussian that ``(mu, cov)`` spells.

``BoxMeasure`` is the uniform measure on a box, ``GaussianMixture`` a weighted sum of Gaussians,
any of which may have zero covariance (a point mass: an empirical measure is a mixture of those).
For the kernel ``h^2 N(. | ., diag(w^2))`` both keep the kernel mean and the prior variance of the
integral in closed form (include/bqhip.h, bq_gp_integral_box and bq_gp_integral_mix).  The objects
are checked when they are made and cannot be changed afterwards; ``engine.Fit.integral``,
``gp.GP.integral`` and the designs take one wherever they take ``mu``, with no ``cov``.
"""
import numpy as np

MAX_COMPONENTS = 64  # BQ_MEASURE_MAX_COMP


def _frozen(a, order):
    a = np.array(a, dtype=np.float64, order=order)
    a.setflags(write=False)
    return a


class Measure(object):
    """What the measures share: ``d``, the dimension; ``key``, bytes that two measures share
    exactly when they are the same measure (the kind is part of it); no attribute can be set."""
    __slots__ = ("_d", "_key")

    @property
    def d(self):
        return self._d

    @property
    def key(self):
        return self._key

    def __setattr__(self, name, value):
        raise AttributeError("a measure is immutable")

    def __delattr__(self, name):
        raise AttributeError("a measure is immutable")

    def _set(self, **kw):
        for k, v in kw.items():
            object.__setattr__(self, k, v)

    def __eq__(self, other):
        return isinstance(other, Measure) and self.key == other.key

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self.key)


class BoxMeasure(Measure):
    """The uniform measure on ``prod_k [lo_k, hi_k]``, density 1 / volume.  ``lo`` and ``hi`` are
    scalars or (d,) vectors, finite, with ``lo < hi`` on every axis."""
    __slots__ = ("_lo", "_hi")

    def __init__(self, lo, hi):
        lo = _frozen(np.atleast_1d(lo), "C")
        hi = _frozen(np.atleast_1d(hi), "C")
        if lo.ndim != 1 or lo.shape != hi.shape or lo.size < 1:
            raise ValueError("lo and hi must be vectors of one length")
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
            raise ValueError("the box's ends must be finite")
        if not np.all(lo < hi):
            raise ValueError("the box needs lo < hi on every axis")
        self._set(_lo=lo, _hi=hi, _d=int(lo.size), _key=b"box" + lo.tobytes() + hi.tobytes())

    @property
    def lo(self):
        return self._lo

    @property
    def hi(self):
        return self._hi

    def __reduce__(self):
        return (BoxMeasure, (self._lo, self._hi))

    def __repr__(self):
        return "BoxMeasure(%r, %r)" % (self._lo.tolist(), self._hi.tolist())


class GaussianMixture(Measure):
    """``sum_c weights_c N(means_c, covs_c)``.  ``weights``: (C,), finite, >= 0, not all zero, used
    as given and not normalised; ``means``: (C, d), or (C,) in one dimension; ``covs``: (C, d, d),
    or (C,) variances in one dimension, each symmetric, any of which may be zero (a point mass).
    At most ``MAX_COMPONENTS`` components.  Whether ``diag(w^2)`` plus a covariance is positive
    definite depends on the kernel, so the integral that uses the measure checks it."""
    __slots__ = ("_weights", "_means", "_covs")

    def __init__(self, weights, means, covs):
        wts = _frozen(np.atleast_1d(weights), "C")
        if wts.ndim != 1 or not 1 <= wts.size <= MAX_COMPONENTS:
            raise ValueError("a mixture has 1..%d components" % MAX_COMPONENTS)
        C = wts.size
        mu = np.asarray(means, dtype=np.float64)
        if mu.ndim == 1 and mu.shape == (C,):
            mu = mu[:, None]
        if mu.ndim != 2 or mu.shape[0] != C or mu.shape[1] < 1:
            raise ValueError("means must be C x d")
        d = mu.shape[1]
        cov = np.asarray(covs, dtype=np.float64)
        if cov.ndim == 1 and d == 1 and cov.shape == (C,):
            cov = cov[:, None, None]
        if cov.shape != (C, d, d):
            raise ValueError("covs must be C x d x d")
        if not (np.all(np.isfinite(wts)) and np.all(np.isfinite(mu)) and np.all(np.isfinite(cov))):
            raise ValueError("the mixture's weights, means and covariances must be finite")
        if np.any(wts < 0):
            raise ValueError("the mixture's weights must not be negative")
        if not wts.sum() > 0:
            raise ValueError("the mixture's weights sum to zero")
        if not np.array_equal(cov, cov.transpose(0, 2, 1)):
            raise ValueError("every covariance must be symmetric")
        mu, cov = _frozen(mu, "C"), _frozen(cov, "C")
        self._set(_weights=wts, _means=mu, _covs=cov, _d=int(d),
                  _key=b"mix" + np.int64(C).tobytes() + wts.tobytes() + mu.tobytes() +
                  cov.tobytes())

    @property
    def weights(self):
        return self._weights

    @property
    def means(self):
        """(C, d): row c is component c's mean -- the d x C column-major block of the C ABI."""
        return self._means

    @property
    def covs(self):
        """(C, d, d): the C ABI's C column-major d x d blocks (each is symmetric)."""
        return self._covs

    def __len__(self):
        return int(self._weights.size)

    def __reduce__(self):
        return (GaussianMixture, (self._weights, self._means, self._covs))

    def __repr__(self):
        return "GaussianMixture(%d components, d = %d)" % (len(self), self._d)
