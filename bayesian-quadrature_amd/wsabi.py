"""Square-root-warped Bayesian quadrature (WSABI-L, Gunter et al. 2014) over the device engine.

For an integrand ``l(x) >= 0`` -- a likelihood -- an unconstrained GP on l goes negative between
the samples.  ``SqrtBQ`` models ``g = sqrt(2 (l - alpha0))`` with one zero-mean GP and linearises
``l = alpha0 + g^2 / 2`` about the posterior mean m of g.  Then l is a GP again, with mean
``alpha0 + m^2 / 2 >= alpha0`` and covariance ``m(x) Sigma(x, x') m(x')``, and for the Gaussian
kernel and a Gaussian measure its integral is closed form (gp.GP.sq_integral, bq_gp_sqintegral):
no log-GP, no candidate points, no second GP.
"""
import numpy as np

from .gp import GP

DTYPE = np.float64


class SqrtBQ(object):
    """Estimate ``Z = int l(x) N(x | x_mean, x_cov) dx`` from samples (x, l) with l >= alpha0 >= 0
    by square-root-warped Bayesian quadrature: one ``GP`` (``self.gp``) with the kernel object
    ``kernel`` and noise ``s`` on ``sqrt(2 (l - alpha0))``.  ``alpha0`` defaults to 0.8 min l;
    ValueError for an l below it."""

    def __init__(self, x, l, kernel, s, x_mean, x_cov, alpha0=None):
        x = np.array(x, dtype=DTYPE)
        l = np.array(l, dtype=DTYPE)
        if x.ndim != 1 or l.ndim != 1:
            raise ValueError("invalid number of dimensions for x or l")
        if x.shape != l.shape:
            raise ValueError("shape mismatch for x and l")
        if x.size == 0:
            raise ValueError("no samples")
        self.x_mean = np.array(np.atleast_1d(x_mean), dtype=DTYPE)
        self.x_cov = np.array(np.atleast_2d(x_cov), dtype=DTYPE)
        if self.x_mean.shape != (1,) or self.x_cov.shape != (1, 1):
            raise ValueError("the prior must be one-dimensional")
        self.alpha0 = self._alpha0(l, alpha0)
        self.x, self.l = x, l
        self.gp = GP(kernel, x, self._warp(l), s=s)

    @staticmethod
    def _alpha0(l, alpha0):
        a = 0.8 * float(np.min(l)) if alpha0 is None else float(alpha0)
        if not np.isfinite(a):
            raise ValueError("alpha0 must be finite")
        if (l < a).any():
            raise ValueError("l contains values below alpha0 = %g" % a)
        return a

    def _warp(self, l):
        return np.sqrt(2.0 * (l - self.alpha0))

    # ---------------------------------------------------------- posterior of l
    def l_mean(self, x):
        """alpha0 + m(x)^2 / 2: never below alpha0."""
        m = self.gp.mean(x)
        return self.alpha0 + 0.5 * m * m

    def l_var(self, x):
        """m(x)^2 v(x), the marginal variance of the linearised l (negatives of v clamped)."""
        m, v = self.gp.mean_var(x)
        return m * m * np.maximum(v, 0.0)

    # --------------------------------------------------------------- integral
    def integral(self):
        """(mean, var) of ``int l(x) N(x | x_mean, x_cov) dx``: alpha0 + sq / 2 and the variance
        of the linearised integral (gp.GP.sq_integral), latent and not clamped."""
        sq, var = self.gp.sq_integral(self.x_mean, self.x_cov)
        return self.alpha0 + 0.5 * sq, var

    def design(self, x_c, q, noisy=True, tol=0.0, return_info=False):
        """The indices of the (at most) ``q`` entries of ``x_c`` whose evaluation lowers the
        variance of ``integral`` the most, one at a time with the posterior mean held
        (gp.GP.sq_integral_design)."""
        return self.gp.sq_integral_design(x_c, q, self.x_mean, self.x_cov, noisy=noisy, tol=tol,
                                          return_info=return_info)

    # ------------------------------------------------------------ acquisition
    def _prior(self, x):
        mu, var = float(self.x_mean[0]), float(self.x_cov[0, 0])
        p = np.exp(-0.5 * (x - mu) ** 2 / var) / np.sqrt(2.0 * np.pi * var)
        return p, -p * (x - mu) / var

    def acquisition(self, x):
        """pi(x)^2 m(x)^2 v(x): the prior-weighted variance of the linearised l, WSABI's
        uncertainty-sampling acquisition."""
        x = np.atleast_1d(np.asarray(x, dtype=DTYPE))
        m, v = self.gp.mean_var(x)
        p, _ = self._prior(x)
        return p * p * m * m * v

    def acquisition_grad(self, x):
        """(acquisition, its gradient in x) from one device call (gp.GP.mean_var_grad)."""
        x = np.atleast_1d(np.asarray(x, dtype=DTYPE))
        m, v, dm, dv = self.gp.mean_var_grad(x)
        p, dp = self._prior(x)
        a = p * p * m * m * v
        return a, 2.0 * p * dp * m * m * v + p * p * (2.0 * m * dm * v + m * m * dv)

    # ----------------------------------------------------------- observations
    def add_observation(self, x_a, l_a):
        """Add samples.  They are appended to the device fit in place (gp.GP.append) with
        targets sqrt(2 (l_a - alpha0)).  An ``l_a`` below alpha0 cannot be warped: alpha0 is then
        set anew to 0.8 times the smallest l seen and the GP gets new targets at all its points,
        which refits it."""
        x_a = np.atleast_1d(np.array(x_a, dtype=DTYPE))
        l_a = np.atleast_1d(np.array(l_a, dtype=DTYPE))
        if x_a.ndim != 1 or x_a.shape != l_a.shape:
            raise ValueError("shape mismatch for x_a and l_a")
        if x_a.size == 0:
            return
        x, l = np.concatenate([self.x, x_a]), np.concatenate([self.l, l_a])
        if (l_a < self.alpha0).any():
            self.alpha0 = 0.8 * float(np.min(l))
            self.gp.x = x
            self.gp.y = self._warp(l)
        else:
            self.gp.append(x_a, self._warp(l_a))
        self.x, self.l = x, l
