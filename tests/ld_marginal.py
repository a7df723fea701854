"""References, float64 yardsticks, cases and bars of the marginal of a fit (csrc/marginal.h;
include/bqhip.h: bq_gp_marginal, bq_gp_marginal_box, bq_marginal_K, bq_marginal_K_box).  A helper
module beside ld_closed_forms.py and ld_measures.py, whose primitives, units and margin it uses:
test_gp_marginal.py holds the device to it, test_gp_marginal_host.py holds this module to
independent derivations (mpmath quadrature), on the CPU.

With S the kept and I the integrated axes, W_S and W_I the blocks of diag(w^2):
  Gaussian N(mu, Sigma): B = Sigma_IS Sigma_SS^-1, m(q) = mu_I + B (q - mu_S), Sigma_c = Sigma_II -
      B Sigma_SI, pi_S(q) = N(q | mu_S, Sigma_SS),
      c(q, x_j) = h^2 pi_S(q) N(q | x_jS, W_S) N(x_jI | m(q), W_I + Sigma_c),
      P(q, q')  = h^2 N(q | q', W_S) pi_S(q) pi_S(q') N(m(q) - m(q') | 0, W_I + 2 Sigma_c);
  box prod [lo, hi]:
      c(q, x_j) = 1[q in box_S] / vol_S N(q | x_jS, W_S) kappa_box,I(x_jI),
      P(q, q')  = 1[q, q' in box_S] / vol_S^2 N(q | q', W_S) kk_box,I.

References: long double -- the Gaussian's three log densities by ld_closed_forms.ld_log_density and
summed before one exp; the box's kappa and kk by ld_measures' mpmath forms at 50 digits.
Yardsticks: the straightforward numpy restatement in float64 -- numpy's inverse and Cholesky, three
log densities, one exp; ld_measures.f64_box_kappa / f64_box_kk.  Their error against the reference
is the ``r`` of the bars, in ld_closed_forms.entry_units; the device gets MARGIN max(r, 4 eps)."""
import functools

import numpy as np

from ld_closed_forms import (EPS, LD, MARGIN, _f64_logn, _ld_inv, _logs, all_normal,  # noqa: F401
                             entry_units, f64_gram, integral_bar, ld_gram, ld_log_density)
from ld_measures import f64_box_kappa, f64_box_kk, mp_box_kappa, mp_box_kk

H = 0.7
DIMS = (2, 3, 5, 8)
MS = (1, 63, 65)
NS = (1, 255, 257)
GAUSS_FAMILIES = ("corr", "diag", "tight", "flat")


def split(d, axes):
    S = sorted(int(a) for a in axes)
    return S, [k for k in range(d) if k not in S]


def keep_sets(d):
    """The kept-axes sets of the per-entry tests: the first axis, the last, {0, d - 1} where d >= 3,
    all but one axis (at d = 8 the first set is the one with |I| = 7)."""
    sets = [(0,), (d - 1,)]
    if d >= 3:
        sets.append((0, d - 1))
    sets.append(tuple(k for k in range(d) if k != 1 % d))
    out = []
    for s in sets:
        if s not in out and 1 <= len(s) <= d - 1:
            out.append(s)
    return out


# ---- long double ----------------------------------------------------------------------------
def _blocks(cov, S, I, T):
    cov = np.asarray(cov).astype(T)
    return cov[np.ix_(S, S)], cov[np.ix_(I, S)], cov[np.ix_(I, I)]


def ld_marg_gauss(xq, x, h, w, axes, mu, cov, want_P=True):
    """(c, P): long double, (M, n) and (M, M); xq is (|S|, M) in ascending axis order, x is d x n."""
    d = x.shape[0]
    S, I = split(d, axes)
    w, mu = np.asarray(w).astype(LD), np.asarray(mu).astype(LD)
    Sss, Sis, Sii = _blocks(cov, S, I, LD)
    B = Sis @ _ld_inv(Sss)
    Sc = Sii - B @ Sis.T
    Sc = (Sc + Sc.T) / 2
    WS, WI = np.diag(w[S] ** 2), np.diag(w[I] ** 2)
    q, xl = np.asarray(xq).astype(LD), np.asarray(x).astype(LD)
    zq = q - mu[S][:, None]
    lpi = ld_log_density(zq, Sss)
    M, n = q.shape[1], xl.shape[1]
    c = np.empty((M, n), dtype=LD)
    for i in range(M):
        m = mu[I] + B @ zq[:, i]
        c[i] = _logs(h) + lpi[i] + ld_log_density(xl[S] - q[:, i:i + 1], WS) + \
            ld_log_density(xl[I] - m[:, None], WI + Sc)
    if not want_P:
        return np.exp(c), None
    P = np.empty((M, M), dtype=LD)
    for i in range(M):
        dq = q - q[:, i:i + 1]
        P[i] = _logs(h) + lpi[i] + lpi + ld_log_density(dq, WS) + ld_log_density(B @ dq, WI + 2 * Sc)
    return np.exp(c), np.exp(P)


def _inside(xq, lo, hi, S):
    xq = np.asarray(xq, dtype=np.float64)
    return np.all((xq >= np.asarray(lo)[S][:, None]) & (xq <= np.asarray(hi)[S][:, None]), axis=0)


def ld_marg_box(xq, x, h, w, axes, lo, hi, want_P=True):
    d = x.shape[0]
    S, I = split(d, axes)
    w, lo, hi = (np.asarray(v, dtype=np.float64) for v in (w, lo, hi))
    ins = _inside(xq, lo, hi, S).astype(LD)
    vol = np.prod((hi[S].astype(LD) - lo[S].astype(LD)))
    kap = mp_box_kappa(np.asarray(x)[I], h, w[I], lo[I], hi[I])
    c = ins[:, None] / vol * ld_gram(xq, np.asarray(x)[S], 1.0, w[S]) * kap[None, :]
    if not want_P:
        return c, None
    P = ins[:, None] * ins[None, :] / (vol * vol) * ld_gram(xq, xq, 1.0, w[S]) * \
        mp_box_kk(h, w[I], lo[I], hi[I])
    return c, P


# ---- float64: the straightforward restatement -----------------------------------------------
def f64_marg_gauss(xq, x, h, w, axes, mu, cov, want_P=True):
    d = x.shape[0]
    S, I = split(d, axes)
    w, mu = np.asarray(w, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    Sss, Sis, Sii = _blocks(cov, S, I, np.float64)
    B = Sis @ np.linalg.inv(Sss)
    Sc = Sii - B @ Sis.T
    Sc = 0.5 * (Sc + Sc.T)
    WS, WI = np.diag(w[S] ** 2), np.diag(w[I] ** 2)
    q, x = np.asarray(xq, dtype=np.float64), np.asarray(x, dtype=np.float64)
    zq = q - mu[S][:, None]
    lpi = _f64_logn(zq, Sss)
    M, n = q.shape[1], x.shape[1]
    c = np.empty((M, n))
    for i in range(M):
        m = mu[I] + B @ zq[:, i]
        c[i] = lpi[i] + _f64_logn(x[S] - q[:, i:i + 1], WS) + _f64_logn(x[I] - m[:, None], WI + Sc)
    if not want_P:
        return h * h * np.exp(c), None
    P = np.empty((M, M))
    for i in range(M):
        dq = q - q[:, i:i + 1]
        P[i] = lpi[i] + lpi + _f64_logn(dq, WS) + _f64_logn(B @ dq, WI + 2 * Sc)
    return h * h * np.exp(c), h * h * np.exp(P)


def f64_marg_box(xq, x, h, w, axes, lo, hi, want_P=True):
    d = x.shape[0]
    S, I = split(d, axes)
    w, lo, hi = (np.asarray(v, dtype=np.float64) for v in (w, lo, hi))
    ins = _inside(xq, lo, hi, S).astype(np.float64)
    vol = np.prod(hi[S] - lo[S])
    kap = f64_box_kappa(np.asarray(x, dtype=np.float64)[I], h, w[I], lo[I], hi[I])
    c = ins[:, None] / vol * f64_gram(xq, np.asarray(x)[S], 1.0, w[S]) * kap[None, :]
    if not want_P:
        return c, None
    P = ins[:, None] * ins[None, :] / (vol * vol) * f64_gram(xq, xq, 1.0, w[S]) * \
        f64_box_kk(h, w[I], lo[I], hi[I])
    return c, P


# ---- cases ------------------------------------------------------------------------------------
def lengths(d):
    return 0.7 * np.random.RandomState(31 * d + 4).uniform(0.9, 1.1, d)


def _corr(d, rho):
    return (1.0 - rho) * np.eye(d) + rho * np.ones((d, d))


@functools.lru_cache(maxsize=None)
def gauss_params(fam, d, axes):
    """(w, mu, cov) of a family for a set of kept axes (tight and flat speak about the
    integrated axes, so the measure depends on the set)."""
    S, I = split(d, axes)
    w = lengths(d)
    rs = np.random.RandomState(17 * d + len(fam))
    mu = 0.4 * np.where(np.arange(d) % 2 == 0, 1.0, -0.5)          # off-centre
    sd = np.full(d, 1.5)
    if fam == "corr":
        C = _corr(d, 0.3)
    elif fam == "diag":
        sd, C = rs.uniform(0.5, 2.0, d), np.eye(d)
    elif fam == "tight":     # Sigma_c a thousand times below w_I^2
        sd[S], C = 1.0, _corr(d, 0.3)
        sd[I] = np.sqrt(1e-3) * w[I]
    else:                    # flat: Sigma_II = 1e4 w_I^2
        sd[I], C = 100.0 * w[I], _corr(d, 0.3)
    cov = sd[:, None] * C * sd[None, :]
    return w, mu, 0.5 * (cov + cov.T)


def reach(d, w):
    """Half the span of the points about mu: at the planted far pair (q at one corner, x at the
    opposite one) every axis adds at most (2 R)^2 / (2 w^2) to the exponent, 520 in all -- about
    1e-226 before pi_S, and a normal number after it."""
    return float(np.min(w)) * np.sqrt(520.0 / (2.0 * d))


M_MAX, N_MAX = max(MS), max(NS)


@functools.lru_cache(maxsize=None)
def _gauss_full(fam, d, axes):
    S, I = split(d, axes)
    w, mu, cov = gauss_params(fam, d, axes)
    rs = np.random.RandomState(1000 * d + 10 * len(S) + S[0] + len(fam))
    R = reach(d, w)
    x = np.asfortranarray(mu[:, None] + R * rs.uniform(-1.0, 1.0, (d, N_MAX)))
    xq = mu[S][:, None] + R * rs.uniform(-1.0, 1.0, (len(S), M_MAX))
    x[:, 0], xq[:, 0] = mu - R, mu[S] + R                            # the far pair
    x[I, 0] = mu[I] - 2.0 * R                    # (2 R from m(q) where Sigma_c and B are small)
    return (x, xq) + ld_marg_gauss(xq, x, H, w, axes, mu, cov) + \
        f64_marg_gauss(xq, x, H, w, axes, mu, cov)


def _case(kind, fam, d, axes, M, n, full, live, extra):
    """The first M query points and n points of the full draw (the far pair is the first of
    each), the reference, the yardstick's r for the cross matrix and r_p for the prior."""
    x, xq, ref, Pref, f64, P64 = full
    live = live[:M]
    x, xq = np.asfortranarray(x[:, :n]), np.ascontiguousarray(xq[:, :M])
    ref, Pref, f64, P64 = ref[:M, :n][live], Pref[:M, :M], f64[:M, :n][live], P64[:M, :M]
    off = np.outer(live, live)
    case = dict(kind=kind, fam=fam, d=d, axes=axes, x=x, xq=xq, h=H, w=lengths(d), live=live,
                ref=ref, P=Pref, pdiag=np.diag(Pref)[live], f64=f64, P64=P64,
                r=float(np.max(entry_units(f64, ref))),
                r_p=float(np.max(entry_units(P64[off], Pref[off]))))
    case.update(extra)
    return case


@functools.lru_cache(maxsize=None)
def gauss_case(fam, d, axes, M=M_MAX, n=N_MAX):
    w, mu, cov = gauss_params(fam, d, axes)
    return _case("gauss", fam, d, axes, M, n, _gauss_full(fam, d, axes),
                 np.ones(M_MAX, dtype=bool), dict(mu=mu, cov=cov))


BOX_LO, BOX_HI = -2.0, 3.0


@functools.lru_cache(maxsize=None)
def _box_full(d, axes):
    S, I = split(d, axes)
    w = lengths(d)
    lo, hi = np.full(d, BOX_LO), np.full(d, BOX_HI)
    rs = np.random.RandomState(2000 * d + 10 * len(S) + S[0])
    x = np.asfortranarray(rs.uniform(-3.0, 4.0, (d, N_MAX)))
    xq = rs.uniform(BOX_LO, BOX_HI, (len(S), M_MAX))
    for i in range(M_MAX):
        a = i % len(S)
        if i % 3 == 1:
            xq[a, i] = BOX_LO if (i // 3) % 2 else BOX_HI
        elif i % 3 == 2:
            xq[a, i] = BOX_HI + 0.5 if (i // 3) % 2 else BOX_LO - 1e-9
    return (x, xq) + ld_marg_box(xq, x, H, w, axes, lo, hi) + f64_marg_box(xq, x, H, w, axes, lo, hi)


@functools.lru_cache(maxsize=None)
def box_case(d, axes, M=M_MAX, n=N_MAX):
    """Box ``mild`` (ld_measures' box): query point i inside for i % 3 == 0, on a face for
    i % 3 == 1 (one kept coordinate exactly an end), outside for i % 3 == 2.  ``live`` marks the
    rows whose reference is not zero; ref and pdiag hold those rows only."""
    S, I = split(d, axes)
    lo, hi = np.full(d, BOX_LO), np.full(d, BOX_HI)
    full = _box_full(d, axes)
    return _case("box", "mild", d, axes, M, n, full, _inside(full[1], lo, hi, S),
                 dict(lo=lo, hi=hi))


def check_entries(got, case, name="ref", r="r"):
    """The per-entry bar on the live rows of a device (or restated) result, exact zeros on the
    others; returns the largest error in units of the bar."""
    got, live = np.asarray(got), case["live"]
    assert np.isfinite(got).all()
    assert not np.any(got[~live]), "a query point outside the box gives exact zeros"
    worst = float(np.max(entry_units(got[live], case[name]))) / integral_bar(case[r])
    assert worst <= 1.0, (name + " per-entry error over the bar", worst, case[r])
    return worst
