"""References, float64 yardsticks, cases and bars of the kernel means under the uniform measure on a
box and under a mixture of Gaussians (csrc/moments.h: int_K_box_kernel, int_K_mix_kernel; include/
bqhip.h: bq_int_K_box, bq_int_K_mix).  A helper module beside ld_closed_forms.py, whose units and
margin it uses: test_gp_measures.py holds the device to it, test_gp_measures_host.py holds this
module to independent derivations, on the CPU.

References.  Box: at 50 digits with mpmath, kappa = h^2 prod_k (ncdf((hi - t) / w) - ncdf((lo - t)
/ w)) / L, the difference taken between the two small values where both arguments are positive
(ncdf(-a) - ncdf(-b): the same number, without 1 - tiny at 20 w from the box), rounded to long
double; kk from I_k = L erf(L / (sqrt2 w)) + w sqrt(2 / pi) expm1(-L^2 / (2 w^2)) at 50 digits.
Mixture: long-double sums of ld_closed_forms.ld_int_K over the components, and for kk over the
pairs (the measure N(mu_c', S_c + S_c') at the point mu_c).

Yardsticks, float64.  Box: the sign-branched scipy.special form of the contract -- with a = (lo -
t) / (sqrt2 w), b = (hi - t) / (sqrt2 w): (erfc(a) - erfc(b)) / 2 for a > 0, (erfc(-b) - erfc(-a))
/ 2 for b < 0, else (erf(b) + erf(-a)) / 2 -- and the expm1 form of kk.  Mixture:
ld_closed_forms.f64_stable_int_K summed over the components.  Their error against the reference is
the ``r`` of the bars, in ld_closed_forms' units; the device gets MARGIN max(r, 4 eps)."""
import functools

import mpmath
import numpy as np
import scipy.special as sp

from ld_closed_forms import (EPS, LD, MARGIN, all_normal, entry_units, f64_stable_int_K,  # noqa: F401
                             integral_bar, ld_int_K)

DPS = 50
DIMS = (1, 2, 3, 8)
SIZES = (1, 255, 257)
N_MAX = max(SIZES)
N_HOST = 40
H = 0.7


def _ld(v):
    return LD(mpmath.nstr(v, 30, min_fixed=0, max_fixed=0))


# ---- the box ------------------------------------------------------------------------------------
def mp_dphi(t, lo, hi, w):
    """Phi((hi - t) / w) - Phi((lo - t) / w) at the working precision, from exact inputs."""
    t, lo, hi, w = (mpmath.mpf(float(v)) for v in (t, lo, hi, w))
    a, b = (lo - t) / w, (hi - t) / w
    if a > 0:
        return mpmath.ncdf(-a) - mpmath.ncdf(-b)
    return mpmath.ncdf(b) - mpmath.ncdf(a)


def mp_box_kappa(x, h, w, lo, hi):
    """(n,) long double: kappa at the columns of x (d x n)."""
    x = np.asarray(x, dtype=np.float64)
    d, n = x.shape
    out = np.empty(n, dtype=LD)
    with mpmath.workdps(DPS):
        h2 = mpmath.mpf(float(h)) ** 2
        for i in range(n):
            v = h2
            for k in range(d):
                v *= mp_dphi(x[k, i], lo[k], hi[k], w[k]) / \
                    (mpmath.mpf(float(hi[k])) - mpmath.mpf(float(lo[k])))
            out[i] = _ld(v)
    return out


def mp_box_kk(h, w, lo, hi):
    with mpmath.workdps(DPS):
        v = mpmath.mpf(float(h)) ** 2
        for k in range(len(w)):
            L = mpmath.mpf(float(hi[k])) - mpmath.mpf(float(lo[k]))
            wk = mpmath.mpf(float(w[k]))
            I = L * mpmath.erf(L / (mpmath.sqrt(2) * wk)) + \
                wk * mpmath.sqrt(2 / mpmath.pi) * mpmath.expm1(-L * L / (2 * wk * wk))
            v *= I / (L * L)
        return _ld(v)


def f64_box_kappa(x, h, w, lo, hi):
    x = np.asarray(x, dtype=np.float64)
    out = np.full(x.shape[1], h * h)
    for k in range(x.shape[0]):
        rw = 1.0 / (np.sqrt(2.0) * w[k])
        a, b = (lo[k] - x[k]) * rw, (hi[k] - x[k]) * rw
        with np.errstate(under="ignore"):
            right = 0.5 * (sp.erfc(a) - sp.erfc(b))
            left = 0.5 * (sp.erfc(-b) - sp.erfc(-a))
            mid = 0.5 * (sp.erf(b) + sp.erf(-a))
        out = out * (np.where(a > 0, right, np.where(b < 0, left, mid)) / (hi[k] - lo[k]))
    return out


def f64_box_kk(h, w, lo, hi):
    out = h * h
    for k in range(len(w)):
        L = hi[k] - lo[k]
        r = L / (np.sqrt(2.0) * w[k])
        out *= (L * sp.erf(r) + w[k] * np.sqrt(2.0 / np.pi) * np.expm1(-r * r)) / (L * L)
    return out


BOX_FAMILIES = ("mild", "edge", "far", "wide", "narrow")


def box_dims(fam):
    return (1, 2, 3) if fam == "far" else DIMS


@functools.lru_cache(maxsize=None)
def box_params(fam, d):
    """(w, lo, hi, draw): draw(rs, n) gives d x n points.  Every kappa is a normal number (asserted
    on the reference): the spans are chosen for it."""
    rs = np.random.RandomState(31 * d + len(fam))
    one = np.ones(d)
    if fam == "mild":      # a box of a few length scales, points inside and around it
        w = 0.7 * rs.uniform(0.9, 1.1, d)
        return w, -2.0 * one, 3.0 * one, lambda r, n: r.uniform(-4.0, 5.0, (d, n))
    if fam == "edge":      # a sharp box: points inside, on the edge's width and 4 w outside
        w = 0.05 * one
        return w, 0.0 * one, 1.0 * one, lambda r, n: r.uniform(-0.2, 1.2, (d, n))
    if fam == "far":       # up to 20 w outside on every axis: both erfc deep in one tail
        w = 0.1 * one
        return w, -1.0 * one, 1.0 * one, lambda r, n: r.uniform(-3.0, 3.0, (d, n))
    if fam == "wide":      # L / w = 2e3: inside dPhi is 1 to the last bit, the edges are 5 w wide
        w = 1e-3 * one

        def draw(r, n):
            x = r.uniform(-1.0, 1.0, (d, n))
            near = r.rand(d, n) < 0.5
            side = np.where(r.rand(d, n) < 0.5, -1.0, 1.0)
            return np.where(near, side + 1e-3 * r.uniform(-5.0, 5.0, (d, n)), x)
        return w, -1.0 * one, 1.0 * one, draw
    # narrow: L / w = 1e-3, the sum erf(b) + erf(-a) cancels 3 digits (the contract's form)
    w = 0.7 * one
    lo = 0.3 * one
    return w, lo, lo + 1e-3 * w, lambda r, n: r.uniform(-2.0, 3.0, (d, n))


@functools.lru_cache(maxsize=None)
def _box_full(fam, d, n):
    w, lo, hi, draw = box_params(fam, d)
    x = np.asfortranarray(draw(np.random.RandomState(7 * d + n), n))
    return x, mp_box_kappa(x, H, w, lo, hi)


@functools.lru_cache(maxsize=None)
def box_case(fam, d, n):
    """One device case: the first n of the family's N_MAX points (the host's N_HOST points are a
    draw of their own), the reference, the yardstick's r, and kk with its own r."""
    w, lo, hi, _ = box_params(fam, d)
    x, ref = _box_full(fam, d, N_HOST if n == N_HOST else N_MAX)
    x, ref = np.asfortranarray(x[:, :n]), ref[:n]
    kk = mp_box_kk(H, w, lo, hi)
    return dict(x=x, h=H, w=w, lo=lo, hi=hi, ref=ref, kk=kk,
                r=float(np.max(entry_units(f64_box_kappa(x, H, w, lo, hi), ref))),
                r_kk=float(abs(LD(f64_box_kk(H, w, lo, hi)) - kk) / kk))


# ---- the mixture --------------------------------------------------------------------------------
def ld_mix_kappa(x, h, w, pi, mu, cov):
    """(n,) long double; mu: C x d, cov: C x d x d."""
    out = 0
    for c in range(len(pi)):
        out = out + LD(pi[c]) * ld_int_K(x, h, w, mu[c], cov[c])
    return out


def ld_mix_kk(h, w, pi, mu, cov):
    out = LD(0)
    for c in range(len(pi)):
        for e in range(len(pi)):
            out += LD(pi[c]) * LD(pi[e]) * ld_int_K(np.asarray(mu[c])[:, None], h, w, mu[e],
                                                     cov[c] + cov[e])[0]
    return out


def f64_mix_kappa(x, h, w, pi, mu, cov):
    out = 0.0
    for c in range(len(pi)):
        out = out + pi[c] * f64_stable_int_K(x, h, w, mu[c], cov[c])
    return out


def f64_mix_kk(h, w, pi, mu, cov):
    out = 0.0
    for c in range(len(pi)):
        for e in range(len(pi)):
            out += pi[c] * pi[e] * f64_stable_int_K(np.asarray(mu[c])[:, None], h, w, mu[e],
                                                     cov[c] + cov[e])[0]
    return out


MIX_FAMILIES = ("corr1", "corr3", "corr16", "point")


@functools.lru_cache(maxsize=None)
def mix_params(fam, d):
    """(w, pi, mu C x d, cov C x d x d).  corr*: correlated (rho 0.3), off-centre components of
    widths 0.3 .. 1.5, weights that are not normalised; point: three components, the middle one
    with zero covariance."""
    C = {"corr1": 1, "corr3": 3, "corr16": 16, "point": 3}[fam]
    rs = np.random.RandomState(977 * d + C + len(fam))
    w = rs.uniform(0.5, 1.5, d)
    pi = rs.uniform(0.2, 1.5, C)
    mu = rs.uniform(-1.5, 1.5, (C, d))
    sc = rs.uniform(0.3, 1.5, C)
    cov = np.array([s * s * (0.7 * np.eye(d) + 0.3 * np.ones((d, d))) for s in sc])
    if fam == "point":
        cov[1] = 0.0
    return w, pi, mu, cov


@functools.lru_cache(maxsize=None)
def _mix_full(fam, d, n):
    w, pi, mu, cov = mix_params(fam, d)
    x = np.asfortranarray(np.random.RandomState(11 * d + n).uniform(-2.0, 2.0, (d, n)))
    return x, ld_mix_kappa(x, H, w, pi, mu, cov)


@functools.lru_cache(maxsize=None)
def mix_case(fam, d, n):
    w, pi, mu, cov = mix_params(fam, d)
    x, ref = _mix_full(fam, d, N_HOST if n == N_HOST else N_MAX)
    x, ref = np.asfortranarray(x[:, :n]), ref[:n]
    kk = ld_mix_kk(H, w, pi, mu, cov)
    return dict(x=x, h=H, w=w, pi=pi, mu=mu, cov=cov, ref=ref, kk=kk,
                r=float(np.max(entry_units(f64_mix_kappa(x, H, w, pi, mu, cov), ref))),
                r_kk=float(abs(LD(f64_mix_kk(H, w, pi, mu, cov)) - kk) / kk))


def check_kappa(got, case, what):
    """The per-entry bar and kk's; returns the largest error in units of the bar."""
    got = np.asarray(got)
    assert got.shape == case["ref"].shape and np.isfinite(got).all()
    worst = float(np.max(entry_units(got, case["ref"]))) / integral_bar(case["r"])
    assert worst <= 1.0, (what + ": kappa per entry over the bar", worst, case["r"])
    return worst


def check_kk(got, case, what):
    worst = float(abs(LD(got) - case["kk"]) / case["kk"]) / integral_bar(case["r_kk"])
    assert worst <= 1.0, (what + ": kk over the bar", worst, case["r_kk"])
    return worst
