"""Engine: one device context of libbqhip.so behind numpy-in / numpy-out calls.

This is the whole seam between the Python host code (``gp.py``, ``linalg.py``,
``bq.py``) and the HIP kernels.  Status codes are mapped to the exceptions the
reference raises at the same places (linalg_c.pyx:49-53,88-91): not positive
definite -> numpy.linalg.LinAlgError, bad argument -> ValueError, HIP failure ->
RuntimeError.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .measures import BoxMeasure, GaussianMixture, Measure

_dp = L._dp


def _pts(x):
    """Points as d x n, column-major (gauss_c.pyx:116-117)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2:
        raise ValueError("points must be a vector or a d x n matrix")
    return np.asfortranarray(x)


def _wvec(w, d):
    w = np.atleast_1d(np.asarray(w, dtype=np.float64)).ravel().copy()
    if w.shape[0] != d:
        raise ValueError("w has invalid shape")
    return w


def _flat_groups(groups):
    """A sequence of integer index sequences as (idx, start), int64: group g is
    idx[start[g]:start[g + 1]] (bq_gp_lgo).  What the indices may be is the library's to check."""
    try:
        groups = [np.asarray(g) for g in groups]
    except TypeError:
        raise ValueError("groups must be a sequence of integer index sequences")
    for g in groups:
        if g.ndim != 1 or (g.size and g.dtype.kind not in "iu"):
            raise ValueError("every group must be a one-dimensional sequence of integers")
    idx = np.concatenate([g.astype(np.int64) for g in groups]) if groups \
        else np.empty(0, dtype=np.int64)
    start = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum(np.array([g.size for g in groups], dtype=np.int64), out=start[1:])
    return np.ascontiguousarray(idx), start


def _measure_args(m):
    """("_box" | "_mix", the C arguments that stand for (mu, cov)) of a measure object."""
    if isinstance(m, BoxMeasure):
        return "_box", (L.dptr(m.lo), L.dptr(m.hi))
    if isinstance(m, GaussianMixture):
        return "_mix", (len(m), L.dptr(m.weights), L.dptr(m.means), L.dptr(m.covs))
    raise TypeError("unknown measure %r" % (m,))


def _marginal_no_mixture(mu):
    if isinstance(mu, GaussianMixture):
        raise ValueError(
            "a marginal takes a single Gaussian (mu, cov) or a BoxMeasure: the conditional of a "
            "mixture has weights that depend on the kept coordinates, and is not built")


def _marginal_points(xq, axes, d):
    """(keep, xq): the kept axes as d int32 flags (which the library checks for their number) and
    the query points -- (|S|, M), row a on axis axes[a], or (M,) for one axis -- scattered into the
    d x M column-major layout of bq_gp_marginal, NaN in the rows that are never read."""
    try:
        axes = [int(a) for a in np.atleast_1d(np.asarray(axes)).ravel()]
    except (TypeError, ValueError):
        raise ValueError("axes must be integers")
    if any(a < 0 or a >= d for a in axes) or len(set(axes)) != len(axes):
        raise ValueError("axes must be distinct and in 0..%d" % (d - 1))
    keep = np.zeros(d, dtype=np.int32)
    keep[axes] = 1
    xq = np.asarray(xq, dtype=np.float64)
    if xq.ndim == 1 and len(axes) == 1:
        xq = xq[None, :]
    if xq.ndim != 2 or xq.shape[0] != len(axes):
        raise ValueError("query points must be (%d, M), one row per kept axis" % len(axes))
    full = np.full((d, xq.shape[1]), np.nan, order="F")
    full[axes, :] = xq
    return keep, full


def _sq_gaussian_only(mu):
    if isinstance(mu, Measure):
        raise ValueError(
            "square-root-warped quadrature takes a single Gaussian (mu, cov) only: on a box the "
            "prior variance alpha^T Q alpha of the warped integral needs a bivariate normal "
            "distribution function and is not closed form, and for a mixture it is a sum over "
            "pairs of components that is not built")


class Engine(object):
    """A device context.  Not thread-safe; use one per thread / per GPU."""

    def __init__(self, device=0, stream=None, probes=False):
        """probes: run on libbqhip_probe.so (the same engine plus the hardware probes)."""
        self._probe_eng = self if probes else None
        self._lib = L.load_probe_library() if probes else L.load_library()
        self._ctx = C.c_void_p()
        n = C.c_int(0)
        self._lib.bq_device_count(C.byref(n))
        if n.value <= 0:
            raise RuntimeError("no HIP device visible: the MI355X engine cannot run "
                               "(there is no CPU fallback)")
        if device >= n.value:
            raise ValueError("device %d out of range (%d visible)" % (device, n.value))
        if stream is None:
            st = self._lib.bq_ctx_create(int(device), C.byref(self._ctx))
        else:
            st = self._lib.bq_ctx_create_on_stream(int(device), C.c_void_p(stream),
                                                   C.byref(self._ctx))
        if st != L.BQ_OK:
            raise RuntimeError("bq_ctx_create failed with status %d" % st)
        self.device = int(device)

    # -- plumbing ---------------------------------------------------------
    def close(self):
        pe = getattr(self, "_probe_eng", None)
        if pe is not None and pe is not self:
            pe.close()
            self._probe_eng = None
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._lib.bq_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st == L.BQ_OK:
            return
        msg = self._lib.bq_last_error(self._ctx)
        msg = msg.decode() if msg else "status %d" % st
        if st == L.BQ_ERR_NOT_PD:
            raise np.linalg.LinAlgError(msg)
        if st == L.BQ_ERR_BAD_ARG:
            raise ValueError(msg)
        if st == L.BQ_ERR_NOMEM:
            raise MemoryError(msg)
        raise RuntimeError(msg)

    def sync(self):
        self._check(self._lib.bq_ctx_sync(self._ctx))

    def device_count(self):
        n = C.c_int(0)
        self._lib.bq_device_count(C.byref(n))
        return n.value

    def info(self):
        name = C.create_string_buffer(64)
        cus, clk, mem = C.c_int(), C.c_int(), C.c_size_t()
        self._check(self._lib.bq_device_info(self._ctx, name, C.byref(cus), C.byref(mem),
                                             C.byref(clk)))
        return {"name": name.value.decode(), "cus": cus.value, "hbm_bytes": mem.value,
                "clock_khz": clk.value}

    def set_block(self, nb):
        self._check(self._lib.bq_set_block(self._ctx, int(nb)))

    def set_guard(self, on):
        """Test aid: device buffers allocated from now on carry a 4 KiB sentinel band
        (Plan.check_guards reads them back).  Process-wide."""
        self._check(self._lib.bq_set_guard(1 if on else 0))

    def set_lookahead(self, on, min_rows=None):
        """Look-ahead on / off; min_rows: rows of the bulk update below which the sweep goes
        sequential (None keeps the current setting, 0 = look-ahead to the end)."""
        self._check(self._lib.bq_set_lookahead(self._ctx, 1 if on else 0))
        if min_rows is not None:
            self._check(self._lib.bq_set_lookahead_rows(self._ctx, int(min_rows)))

    def config(self):
        """(outer block override, look-ahead on, look-ahead min_rows) as they stand."""
        nb, la, mr = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.bq_get_config(self._ctx, C.byref(nb), C.byref(la), C.byref(mr)))
        return nb.value, bool(la.value), mr.value

    def stats(self):
        """Counters of the context: ``flow_fallbacks`` = single-vector solves re-issued on the
        per-block sweeps after a hand-off of the one-launch sweeps timed out; ``graph_captures`` =
        launch sequences (a plan's pass, a pair's objective, a fit's vector sweeps) captured into
        a hipGraph, ``graph_replays`` = launches of such graphs, ``graph_drops`` = graphs dropped
        because a setter had changed the configuration they were captured under."""
        v = (C.c_int64 * 4)()
        self._check(self._lib.bq_ctx_stats(self._ctx, v, 4))
        return {"flow_fallbacks": int(v[0]), "graph_captures": int(v[1]),
                "graph_replays": int(v[2]), "graph_drops": int(v[3])}

    def trim(self):
        """Release the workspace the batched calls keep between calls."""
        self._check(self._lib.bq_ctx_trim(self._ctx))

    # -- raw device memory -------------------------------------------------

    def alloc(self, nbytes):
        p = C.c_void_p()
        self._check(self._lib.bq_dev_alloc(self._ctx, int(nbytes), C.byref(p)))
        return p

    def free(self, p):
        self._check(self._lib.bq_dev_free(self._ctx, p))

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr) if not arr.flags.f_contiguous else arr
        self._check(self._lib.bq_upload(self._ctx, dptr, arr.ctypes.data_as(C.c_void_p),
                                        arr.nbytes))

    def download(self, arr, dptr):
        self._check(self._lib.bq_download(self._ctx, arr.ctypes.data_as(C.c_void_p), dptr,
                                          arr.nbytes))

    def timer_start(self):
        self._check(self._lib.bq_timer_start(self._ctx))

    def timer_stop_ms(self):
        ms = C.c_float()
        self._check(self._lib.bq_timer_stop_ms(self._ctx, C.byref(ms)))
        return float(ms.value)

    def profile(self, on):
        self._check(self._lib.bq_profile_enable(self._ctx, 1 if on else 0))

    def profile_reset(self):
        self._check(self._lib.bq_profile_reset(self._ctx))

    def timeline(self, fn):
        """Runs fn() under the launch profiler and returns its launches as rows
        (class name, stream, start ms, end ms, work), times since the first launch."""
        self.profile(True)
        self.profile_reset()
        self._check(self._lib.bq_profile_timeline(self._ctx, 1, None, 0, None))
        fn()
        n = C.c_int64(0)
        self._check(self._lib.bq_profile_timeline(self._ctx, 0, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 5))
        self._check(self._lib.bq_profile_timeline(self._ctx, 0, L.dptr(out), n.value, C.byref(n)))
        self.profile(False)
        return [(L.K_CLASSES[int(r[0])], int(r[1]), r[2], r[3], r[4]) for r in out[:n.value]]

    def profile_read(self):
        ms = np.zeros(len(L.K_CLASSES))
        work = np.zeros(len(L.K_CLASSES))
        cnt = np.zeros(len(L.K_CLASSES), dtype=np.int64)
        self._check(self._lib.bq_profile_read(self._ctx, L.dptr(ms),
                                              cnt.ctypes.data_as(L._i64p), L.dptr(work)))
        return {k: {"ms": float(ms[i]), "launches": int(cnt[i]), "work": float(work[i])}
                for i, k in enumerate(L.K_CLASSES)}

    # -- linalg_c drop-ins (host arrays) ------------------------------------
    def cho_factor(self, Cm, Lm):
        """linalg_c.pyx:55-93 semantics; Cm, Lm are F-contiguous n x n."""
        n = Cm.shape[0]
        info = C.c_int64(0)
        self._check(self._lib.bq_cho_factor(self._ctx, L.dptr(Cm), L.dptr(Lm), n,
                                            C.byref(info)))

    def cho_solve(self, Lm, B, X, nrhs):
        self._check(self._lib.bq_cho_solve(self._ctx, L.dptr(Lm), L.dptr(B), L.dptr(X),
                                           Lm.shape[0], int(nrhs)))

    def logdet(self, Lm):
        out = C.c_double()
        self._check(self._lib.bq_logdet(self._ctx, L.dptr(Lm), Lm.shape[0],
                                        C.cast(C.byref(out), _dp)))
        return float(out.value)

    # -- Gram -----------------------------------------------------------------
    def gram(self, x, h, w, s=0.0):
        x = _pts(x)
        d, n = x.shape
        w = _wvec(w, d)
        K = np.empty((n, n), order="F")
        self._check(self._lib.bq_gram_gauss(self._ctx, L.dptr(x), d, n, float(h), L.dptr(w),
                                            float(s), L.dptr(K)))
        return K

    def gram_cross(self, x1, x2, h, w):
        x1, x2 = _pts(x1), _pts(x2)
        d = x1.shape[0]
        if x2.shape[0] != d:
            raise ValueError("dimension mismatch")
        w = _wvec(w, d)
        K = np.empty((x1.shape[1], x2.shape[1]), order="F")
        self._check(self._lib.bq_gram_gauss_cross(self._ctx, L.dptr(x1), x1.shape[1], L.dptr(x2),
                                                  x2.shape[1], d, float(h), L.dptr(w), L.dptr(K)))
        return K

    # -- closed-form integrals (gauss_c), host arrays -------------------------
    @staticmethod
    def _mc(d, mu, cov):
        mu = np.ascontiguousarray(np.atleast_1d(mu), dtype=np.float64)
        cov = np.asfortranarray(np.atleast_2d(cov), dtype=np.float64)
        if mu.shape != (d,):
            raise ValueError("mu has invalid shape")
        if cov.shape != (d, d):
            raise ValueError("cov has invalid shape")
        return mu, cov

    def int_K(self, x, h, w, mu, cov):
        x = _pts(x)
        d, n = x.shape
        w = _wvec(w, d)
        mu, cov = self._mc(d, mu, cov)
        out = np.empty(n)
        self._check(self._lib.bq_int_K(self._ctx, L.dptr(x), d, n, float(h), L.dptr(w), L.dptr(mu),
                                       L.dptr(cov), L.dptr(out)))
        return out

    def int_K_box(self, x, h, w, measure, want_kk=False):
        """kappa(x_i) = int k(x_i, x') dx' / vol over the box of a ``measures.BoxMeasure``, (n,)
        (bq_int_K_box); ``want_kk`` appends kk, the prior variance of the integral."""
        return self._int_K_measure(x, h, w, measure, BoxMeasure, want_kk)

    def int_K_mix(self, x, h, w, measure, want_kk=False):
        """kappa(x_i) = sum_c pi_c int k(x_i, x') N(x' | mu_c, Sigma_c) dx' for a
        ``measures.GaussianMixture``, (n,) (bq_int_K_mix); ``want_kk`` appends kk."""
        return self._int_K_measure(x, h, w, measure, GaussianMixture, want_kk)

    def _int_K_measure(self, x, h, w, measure, kind, want_kk):
        if not isinstance(measure, kind):
            raise TypeError("measure must be a %s" % kind.__name__)
        x = _pts(x)
        d, n = x.shape
        w = _wvec(w, d)
        if measure.d != d:
            raise ValueError("the measure has dimension %d, the points %d" % (measure.d, d))
        out, kk = np.empty(n), C.c_double()
        name, margs = _measure_args(measure)
        self._check(getattr(self._lib, "bq_int_K" + name)(
            self._ctx, L.dptr(x), d, n, float(h), L.dptr(w), *(margs + (
                L.dptr(out), C.byref(kk) if want_kk else None))))
        return (out, float(kk.value)) if want_kk else out

    def marginal_K(self, xq, x, h, w, axes, mu, cov=None):
        """(c, pdiag): the cross matrix c(xq_i, x_j), (M, n), and the prior's diagonal
        P(xq_i, xq_i), (M,), of ``Fit.marginal`` at host points without a fit (bq_marginal_K,
        bq_marginal_K_box).  ``axes`` are the kept axes, ``xq`` is (|S|, M) -- or (M,) for one
        axis --, ``x`` is d x n; (mu, cov) spell a Gaussian, a ``measures.BoxMeasure`` in place
        of mu the box.  ValueError for a ``measures.GaussianMixture``."""
        _marginal_no_mixture(mu)
        x = _pts(x)
        d, n = x.shape
        w = _wvec(w, d)
        keep, xq = _marginal_points(xq, axes, d)
        if isinstance(mu, Measure):
            if cov is not None:
                raise TypeError("a measure object comes without a cov")
            if mu.d != d:
                raise ValueError("the measure has dimension %d, the points %d" % (mu.d, d))
            name, margs = _measure_args(mu)
        else:
            if cov is None:
                raise TypeError("a Gaussian measure needs its cov")
            mu, cov = self._mc(d, mu, cov)
            name, margs = "", (L.dptr(mu), L.dptr(cov))
        M = xq.shape[1]
        out, pdiag = np.empty((M, n), order="F"), np.empty(M)
        self._check(getattr(self._lib, "bq_marginal_K" + name)(
            self._ctx, L.dptr(xq), M, L.dptr(x), n, d, float(h), L.dptr(w),
            keep.ctypes.data_as(L._i32p), *(margs + (L.dptr(out), L.dptr(pdiag)))))
        return out, pdiag

    def int_K1_K2(self, x1, x2, h1, w1, h2, w2, mu, cov):
        x1, x2 = _pts(x1), _pts(x2)
        d = x1.shape[0]
        if x2.shape[0] != d:
            raise ValueError("x2 has invalid shape")
        w1, w2 = _wvec(w1, d), _wvec(w2, d)
        mu, cov = self._mc(d, mu, cov)
        out = np.empty((x1.shape[1], x2.shape[1]), order="F")
        self._check(self._lib.bq_int_K1_K2(self._ctx, L.dptr(x1), x1.shape[1], L.dptr(x2),
                                           x2.shape[1], d, float(h1), L.dptr(w1), float(h2),
                                           L.dptr(w2), L.dptr(mu), L.dptr(cov), L.dptr(out)))
        return out

    def int_int_K1_K2_K1(self, x, h1, w1, h2, w2, mu, cov):
        x = _pts(x)
        d, n = x.shape
        w1, w2 = _wvec(w1, d), _wvec(w2, d)
        mu, cov = self._mc(d, mu, cov)
        out = np.empty((n, n), order="F")
        self._check(self._lib.bq_int_int_K1_K2_K1(self._ctx, L.dptr(x), d, n, float(h1), L.dptr(w1),
                                                  float(h2), L.dptr(w2), L.dptr(mu), L.dptr(cov),
                                                  L.dptr(out)))
        return out

    def int_int_K1_K2(self, x, h1, w1, h2, w2, mu, cov):
        x = _pts(x)
        d, n = x.shape
        w1, w2 = _wvec(w1, d), _wvec(w2, d)
        mu, cov = self._mc(d, mu, cov)
        out = np.empty(n)
        self._check(self._lib.bq_int_int_K1_K2(self._ctx, L.dptr(x), d, n, float(h1), L.dptr(w1),
                                               float(h2), L.dptr(w2), L.dptr(mu), L.dptr(cov),
                                               L.dptr(out)))
        return out

    # -- BQ moments on resident fits (bq_c) -------------------------------------
    def Z_mean(self, fit_l, mu, cov):
        mu, cov = self._mc(fit_l.d, mu, cov)
        out = C.c_double()
        self._check(self._lib.bq_bq_Z_mean(self._ctx, fit_l._handle(), L.dptr(mu), L.dptr(cov),
                                           C.cast(C.byref(out), _dp)))
        return float(out.value)

    def Z_var(self, fit_tl, fit_l, mu, cov):
        mu, cov = self._mc(fit_l.d, mu, cov)
        out = C.c_double()
        self._check(self._lib.bq_bq_Z_var(self._ctx, fit_tl._handle(), fit_l._handle(), L.dptr(mu), L.dptr(cov),
                                          C.cast(C.byref(out), _dp)))
        return float(out.value)

    def esm_batch(self, x_sc, l_sc, ns, x_a, h, w, thresh, mu, cov):
        """(A_a, A_sc_l, status) for every candidate of x_a (1-D); see bq_esm_batch."""
        x_sc = np.ascontiguousarray(x_sc, dtype=np.float64)
        l_sc = np.ascontiguousarray(l_sc, dtype=np.float64)
        x_a = np.ascontiguousarray(x_a, dtype=np.float64)
        mu, cov = self._mc(1, mu, cov)
        M = x_a.shape[0]
        A_a, A_sc_l = np.empty(M), np.empty(M)
        status = np.zeros(M, dtype=np.int32)
        self._check(self._lib.bq_esm_batch(
            self._ctx, L.dptr(x_sc), L.dptr(l_sc), int(ns), x_sc.shape[0], L.dptr(x_a), M,
            float(h), float(w), float(thresh), L.dptr(mu), L.dptr(cov), L.dptr(A_a),
            L.dptr(A_sc_l), status.ctypes.data_as(L._i32p)))
        return A_a, A_sc_l, status

    def esm_border(self, fit_l, ns, x_a, thresh, mu, cov):
        """(A_a, A_sc_l, status) for every candidate of x_a from the RESIDENT factor of
        gp_l (a Fit over (x_sc, l_sc), s = 0): one multi-right-hand-side solve instead of
        one factorisation per candidate; see bq_esm_border."""
        x_a = np.ascontiguousarray(x_a, dtype=np.float64)
        mu, cov = self._mc(1, mu, cov)
        M = x_a.shape[0]
        A_a, A_sc_l = np.empty(M), np.empty(M)
        status = np.zeros(M, dtype=np.int32)
        self._check(self._lib.bq_esm_border(
            self._ctx, fit_l._handle(), int(ns), L.dptr(x_a), M, float(thresh), L.dptr(mu),
            L.dptr(cov), L.dptr(A_a), L.dptr(A_sc_l), status.ctypes.data_as(L._i32p)))
        return A_a, A_sc_l, status

    # -- GP fits --------------------------------------------------------------
    def gp_fit(self, x, y, h, w, s=0.0):
        return Fit(self, x, y, h, w, s)

    def fit_predict(self, x, y, h, w, s, xo):
        """One bordered-Cholesky pass: (mean, var, logml)."""
        x, xo = _pts(x), _pts(xo)
        d, n = x.shape
        M = xo.shape[1]
        if xo.shape[0] != d:
            raise ValueError("dimension mismatch")
        w = _wvec(w, d)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (n,):
            raise ValueError("y has invalid shape")
        mean, var = np.empty(M), np.empty(M)
        logml = C.c_double()
        self._check(self._lib.bq_fit_predict(self._ctx, L.dptr(x), L.dptr(y), d, n, float(h),
                                             L.dptr(w), float(s), L.dptr(xo), M, L.dptr(mean),
                                             L.dptr(var), C.cast(C.byref(logml), _dp)))
        return mean, var, float(logml.value)

    def logml_grid(self, x, y, h, w, s=0.0, chunk=0):
        """log-ML at G hyper-parameter points: h (G,), w (G,) or (G, d)."""
        x = _pts(x)
        d, n = x.shape
        y = np.ascontiguousarray(y, dtype=np.float64)
        h = np.ascontiguousarray(h, dtype=np.float64).ravel()
        G = h.shape[0]
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(G, -1))
        if w.shape[1] == 1 and d > 1:
            w = np.ascontiguousarray(np.repeat(w, d, axis=1))
        if w.shape != (G, d):
            raise ValueError("w has invalid shape")
        out = np.empty(G)
        self._check(self._lib.bq_gp_logml_grid(self._ctx, L.dptr(x), L.dptr(y), d, n, L.dptr(h),
                                               L.dptr(w), float(s), G, L.dptr(out), int(chunk)))
        return out

    def batch_fit_predict(self, x, y, h, w, s, xo):
        """nprob independent problems.  x: (P, n) or (P, d, n); y: (P, n);
        xo: (P, M) or (P, d, M).  Returns mean (P, M), var (P, M), logml (P,),
        status (P,)."""
        x = np.asarray(x, dtype=np.float64)
        xo = np.asarray(xo, dtype=np.float64)
        if x.ndim == 2:
            x = x[:, None, :]
        if xo.ndim == 2:
            xo = xo[:, None, :]
        P, d, n = x.shape
        M = xo.shape[2]
        # each problem's points are d x n column-major = (n, d) C-order
        xb = np.ascontiguousarray(np.transpose(x, (0, 2, 1)))
        xob = np.ascontiguousarray(np.transpose(xo, (0, 2, 1)))
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (P, n) or xo.shape[0] != P or xo.shape[1] != d:
            raise ValueError("shape mismatch")
        w = _wvec(w, d)
        mean, var = np.empty((P, M)), np.empty((P, M))
        logml = np.empty(P)
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bq_batch_fit_predict(
            self._ctx, P, L.dptr(xb), L.dptr(y), d, n, float(h), L.dptr(w), float(s),
            L.dptr(xob), M, L.dptr(mean), L.dptr(var), L.dptr(logml),
            status.ctypes.data_as(L._i32p)))
        return mean, var, logml, status

    def plan(self, nprob, d, n, M):
        return Plan(self, nprob, d, n, M)

    def pair(self, x_s, tl_s, l_s, x_c, x_a, S):
        """The stacked pair of GPs of a BQ object, resident for S hyper-parameter sets
        (bq_pair): ``llh`` without acquisition points, ``esm`` with them."""
        return Pair(self, x_s, tl_s, l_s, x_c, x_a, S)

    # -- probes ----------------------------------------------------------------
    def probe_engine(self):
        """The engine the probe_* methods run on: this one if it was created with probes=True,
        else an engine on libbqhip_probe.so for the same device, created on first use and closed
        with this one (its own context: the probes see the environment's switches, not this
        engine's setters)."""
        if self._probe_eng is None:
            self._probe_eng = Engine(self.device, probes=True)
        return self._probe_eng

    def probe_mfma_f64(self):
        e = self.probe_engine()
        v = C.c_double()
        e._check(e._lib.bq_probe_mfma_f64(e._ctx, C.cast(C.byref(v), _dp)))
        return float(v.value)

    def probe_mfma_variant(self, kind, nacc=8, waves_per_simd=2):
        """TFLOP/s of back-to-back independent MFMAs: kind 0 = v_mfma_f64_16x16x4_f64,
        1 = v_mfma_f64_4x4x4_4b_f64."""
        e = self.probe_engine()
        v = C.c_double()
        e._check(e._lib.bq_probe_mfma_variant(e._ctx, int(kind), int(nacc),
                                              int(waves_per_simd), C.cast(C.byref(v), _dp)))
        return v.value

    def probe_fma_f64(self):
        e = self.probe_engine()
        v = C.c_double()
        e._check(e._lib.bq_probe_fma_f64(e._ctx, C.cast(C.byref(v), _dp)))
        return float(v.value)

    def probe_hbm(self, nbytes=1 << 30):
        e = self.probe_engine()
        a, b = C.c_double(), C.c_double()
        e._check(e._lib.bq_probe_hbm(e._ctx, int(nbytes), C.cast(C.byref(a), _dp),
                                     C.cast(C.byref(b), _dp)))
        return float(a.value), float(b.value)

    def probe_hbm_read8(self, nbytes=1 << 30, reps=4):
        """GB/s of a read-only pass with the single-vector sweeps' access pattern (8 B per
        lane); under ``rocprofv3 --pmc FETCH_SIZE`` a known byte count for that counter."""
        e = self.probe_engine()
        v = C.c_double()
        e._check(e._lib.bq_probe_hbm_read8(e._ctx, int(nbytes), int(reps),
                                           C.cast(C.byref(v), _dp)))
        return float(v.value)

    def probe_gemm(self, m, n, k, lower=0, batch=1, qt=False, reps=20):
        """ms per launch of C (m x n) -= P Q^T (k columns) through the engine's kernel selection."""
        e = self.probe_engine()
        v = C.c_double()
        e._check(e._lib.bq_probe_gemm(e._ctx, int(m), int(n), int(k), int(lower),
                                      int(batch), 1 if qt else 0, int(reps),
                                      C.cast(C.byref(v), _dp)))
        return float(v.value)

    GEMM_KERNELS = ("Lds128", "Lds64", "Lds64QT", "Sub128", "Sub64", "Sub32", "K64x64", "K64x32",
                    "SplitK")

    def probe_gemm_product(self, m, n, k, C_=None, P=None, Q=None, lower=0, batch=1, qt=False, ccut=0,
                           sharing=0, want_fuse=False, j0=0, seed_d=0, rows=False, ldq=0):
        """ONE product C (m x n) -= P (m x k) Q (n x k)^T per batch element on the caller's operands
        (bq_probe_gemm_product), and the route the launch took.  C_, P, Q: Fortran-ordered float64
        arrays whose first axis is the leading dimension and whose columns are the batch elements'
        side by side -- (ldc, n batch), (ldp, k batch), (ldq, k batch), or with qt (Q k-contiguous)
        (ldq, n batch) holding Q^T; C_ is updated in place.  Without operands nothing is launched and
        the route is the engine's answer for the shape (seed_d > 0 only then; ldq: the leading
        dimension Q would have).
        Returns {"kernel", "mfma", "fused", "seeded", "assemble_first", "grid"} and, when the launch
        carried the diagonal factor want_fuse asks for, "dinv" (batch x 64 reciprocal pivots) and
        "info" (per element: 0, or j0 + the 1-based failing column)."""
        m, n, k, batch, ccut, j0, seed_d = (int(v) for v in (m, n, k, batch, ccut, j0, seed_d))
        if m < 16 or m % 16 or n < 16 or n % 16 or k < 8 or k % 8:
            raise ValueError("m and n must be multiples of 16, k of 8")
        if batch < 1 or ccut < 0 or j0 < 0:
            raise ValueError("batch >= 1, ccut >= 0, j0 >= 0")
        if sharing not in (0, 1, 2):
            raise ValueError("sharing must be 0, 1 or 2")
        if seed_d not in (0, 1, 2, 3):
            raise ValueError("seed_d must be 0 .. 3")
        if want_fuse and (m < 64 or n < 64):
            raise ValueError("a fused diagonal factor needs a leading 64 x 64 block")
        if rows and (lower or batch != 1 or seed_d or want_fuse):
            raise ValueError("a sweep's product is one full matrix, unseeded, unfused")
        ops = (C_, P, Q)
        run = any(a is not None for a in ops)
        if run:
            if any(a is None for a in ops):
                raise ValueError("C_, P and Q come together")
            if seed_d:
                raise ValueError("a seeded product is only routed (no operands)")
            for name, a, rows_min, cols in (("C_", C_, m, n * batch), ("P", P, m, k * batch),
                                            ("Q", Q, k if qt else n, (n if qt else k) * batch)):
                if a.dtype != np.float64 or a.ndim != 2 or not a.flags.f_contiguous:
                    raise ValueError("%s must be a Fortran-ordered float64 matrix" % name)
                if a.shape[0] < rows_min or a.shape[1] != cols:
                    raise ValueError("%s must be (ld >= %d, %d)" % (name, rows_min, cols))
        e = self.probe_engine()
        route = np.full(8, -1, dtype=np.int32)
        dinv = np.zeros((batch, 64))
        info = np.full(batch, -1, dtype=np.int32)
        e._check(e._lib.bq_probe_gemm_product(
            e._ctx, L.dptr(C_) if run else None, C_.shape[0] if run else 0,
            L.dptr(P) if run else None, P.shape[0] if run else 0,
            L.dptr(Q) if run else None, Q.shape[0] if run else int(ldq), m, n, k, int(lower), batch,
            1 if qt else 0, ccut, int(sharing), 1 if want_fuse else 0, j0, seed_d, 1 if rows else 0,
            L.dptr(dinv), info.ctypes.data_as(L._i32p), route.ctypes.data_as(L._i32p)))
        out = {"kernel": self.GEMM_KERNELS[route[0]], "mfma": int(route[1]), "fused": bool(route[2]),
               "seeded": bool(route[3]), "assemble_first": bool(route[4]),
               "grid": tuple(int(v) for v in route[5:8])}
        if run and out["fused"]:
            out["dinv"], out["info"] = dinv, info
        return out

    def probe_panel_solve(self, Lfac, X, mode=0, reps=0):
        """X L^-T for a batch of lower-triangular kb x kb factors L (batch, kb, kb) and row blocks
        X (batch, m, kb) through the batched factorisation's panel-solve launches."""
        e = self.probe_engine()
        L_ = np.asarray(Lfac, dtype=np.float64)
        X_ = np.asarray(X, dtype=np.float64)
        batch, kb, _ = L_.shape
        m = X_.shape[1]
        # column-major per problem
        Lf = np.ascontiguousarray(np.transpose(L_, (0, 2, 1)))
        Xf = np.ascontiguousarray(np.transpose(X_, (0, 2, 1)))
        ms = C.c_double()
        e._check(e._lib.bq_probe_panel_solve(e._ctx, int(m), int(kb), int(batch),
                                             L.dptr(Lf), L.dptr(Xf), int(mode), int(reps),
                                             C.cast(C.byref(ms), _dp)))
        if reps > 0:
            return float(ms.value)  # ms per call
        return np.transpose(Xf, (0, 2, 1)).copy()

    SWEEP_KINDS = ("slab", "blocked", "halves", "diag_first")

    def probe_potrf_batch(self, buf, batch, ntot, ncols=None, lda=0, astride=0):
        """The batched Cholesky sweep on the caller's matrices (bq_probe_potrf_batch): buf is a
        flat float64 array of batch * astride doubles (column-major matrices of leading dimension
        lda; 0 = the plans' own strides), factored in place.  Returns (info per matrix,
        (route kind, outer block, scratch used))."""
        e = self.probe_engine()
        if buf.dtype != np.float64 or buf.ndim != 1 or not buf.flags.c_contiguous:
            raise ValueError("buf must be a flat contiguous float64 array")
        ld = int(lda) if lda else self.plan_ld(ntot)
        stride = int(astride) if astride else ld * int(ntot)
        if buf.shape[0] != stride * int(batch):
            raise ValueError("buf holds %d doubles, the batch %d" % (buf.shape[0], stride * batch))
        info = np.full(int(batch), -1, dtype=np.int32)
        route = np.full(3, -1, dtype=np.int32)
        e._check(e._lib.bq_probe_potrf_batch(
            e._ctx, int(batch), int(ntot), int(ntot if ncols is None else ncols), int(lda),
            int(astride), L.dptr(buf), info.ctypes.data_as(L._i32p),
            route.ctypes.data_as(L._i32p)))
        return info, (self.SWEEP_KINDS[route[0]], int(route[1]), bool(route[2]))

    def probe_records(self, A):
        """Both producers of the block-inverse records on one 128 x 128 SPD matrix
        (bq_probe_records).  Returns (factor, the sweep's two records (2, 1088), the resident
        factor's two records (2, 1088), info)."""
        e = self.probe_engine()
        buf = np.array(A, dtype=np.float64, order="F")
        if buf.shape != (128, 128):
            raise ValueError("A must be 128 x 128")
        rs, rr = np.zeros((2, 1088)), np.zeros((2, 1088))
        info = np.full(1, -1, dtype=np.int32)
        e._check(e._lib.bq_probe_records(e._ctx, L.dptr(buf), L.dptr(rs), L.dptr(rr),
                                         info.ctypes.data_as(L._i32p)))
        return buf, rs, rr, int(info[0])

    def probe_first_launch(self, x, y, xo, h, w, s, stamps=False):
        """The first launch of a small system's sweep alone (bq_probe_first_launch): x (B, d, n),
        y (B, n), xo (B, d, M) as a plan takes them.  Returns a dict of what the launch left in
        memory -- "A" (B, ntot, 64), the first block column of every system; "S0" (B, ntot, 64);
        "dinv" (B, record); "info" (B,); "scal" (B, 4) -- over buffers preset to 0xA5 bytes, and
        with stamps (d = 1) "stamps": 16 shader-clock values of workgroup (0, 0)."""
        e = self.probe_engine()
        x = np.asarray(x, dtype=np.float64)
        B, d, n = x.shape
        xo = np.zeros((B, d, 0)) if xo is None else np.asarray(xo, dtype=np.float64)
        M = xo.shape[2]
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (B, n) or xo.shape != (B, d, M):
            raise ValueError("y must be (B, n) and xo (B, d, M)")
        # point-major per problem, as the plans take their inputs
        xf = np.ascontiguousarray(np.transpose(x, (0, 2, 1)))
        xof = np.ascontiguousarray(np.transpose(xo, (0, 2, 1)))
        wv = np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.float64), (d,)))
        ntot = -(-(-(-n // 64) * 64 + M + 1) // 64) * 64
        rec = 2 * (64 + 4 * 256)  # (ntot and rec go along: the library checks both against its own)
        out = {"A": np.empty((B, 64, ntot)), "S0": np.empty((B, 64, ntot)),
               "dinv": np.empty((B, rec)), "info": np.empty(B, dtype=np.int32),
               "scal": np.empty((B, 4))}
        st = np.zeros(16, dtype=np.int64) if stamps else None
        e._check(e._lib.bq_probe_first_launch(
            e._ctx, B, d, n, M, L.dptr(xf), L.dptr(y), L.dptr(xof) if M else None, float(h),
            L.dptr(wv), float(s), ntot, rec, L.dptr(out["A"]), L.dptr(out["S0"]), L.dptr(out["dinv"]),
            out["info"].ctypes.data_as(L._i32p), L.dptr(out["scal"]),
            st.ctypes.data_as(C.POINTER(C.c_int64)) if stamps else None))
        out["A"] = np.transpose(out["A"], (0, 2, 1))
        out["S0"] = np.transpose(out["S0"], (0, 2, 1))
        if stamps:
            out["stamps"] = st
        return out

    SWEEPS = ("forward_rows", "backward_rows", "forward_rows_blk", "inverse_rows", "forward_vec",
              "backward_vec", "forward_vec_flow", "backward_vec_flow")
    ROWS_KINDS = ("step", "fused", "gemm_rows", "blk", "vec_block", "vec_flow")

    def probe_sweep(self, which, Lfac, X, mrows=None, ldl=0):
        """ONE sweep over a resident factor on the caller's factor (bq_probe_sweep).  Lfac: n x n
        lower factor, n a multiple of 64; X: the right-hand sides as rows, a Fortran-ordered
        (ldx, n) float64 array whose first mrows rows (default: all) are solved in place, the others
        only travel; ldl: the factor's leading dimension on the device (0: the engine's own).
        Returns the route: {"kind", "B", "lds", "splitk", "flow_fallbacks"}."""
        e = self.probe_engine()
        Lf = L.f64(Lfac)
        n = Lf.shape[0]
        if Lf.shape != (n, n):
            raise ValueError("Lfac must be square")
        if X.dtype != np.float64 or X.ndim != 2 or not X.flags.f_contiguous or X.shape[1] != n:
            raise ValueError("X must be a Fortran-ordered float64 (ldx, n) array")
        ldx = X.shape[0]
        route = np.full(5, -1, dtype=np.int32)
        e._check(e._lib.bq_probe_sweep(
            e._ctx, self.SWEEPS.index(which), n, L.dptr(Lf), int(ldl),
            int(ldx if mrows is None else mrows), ldx, L.dptr(X), route.ctypes.data_as(L._i32p)))
        return {"kind": self.ROWS_KINDS[route[0]], "B": int(route[1]), "lds": int(route[2]),
                "splitk": int(route[3]), "flow_fallbacks": int(route[4])}

    @staticmethod
    def plan_ld(ntot):
        """Leading dimension of a plan's ntot-row systems (csrc/host.h, pick_ld)."""
        return int(ntot) + (64 if ntot >= 1024 and ntot % 512 == 0 else 0)

    def probe_xcd_hop(self, mode, iters=2000, kib=1):
        """(ns per hand-off, XCC ids of the 16 workgroups, stale payload words) -- see
        bq_probe_xcd_hop in include/bqhip_probe.h."""
        e = self.probe_engine()
        ns, bad = C.c_double(), C.c_int64()
        xcc = np.zeros(16, dtype=np.int32)
        e._check(e._lib.bq_probe_xcd_hop(e._ctx, int(mode), int(iters), int(kib),
                                         C.byref(ns),
                                         xcc.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.byref(bad)))
        return float(ns.value), xcc, int(bad.value)

    def probe_launch(self, n=2000):
        e = self.probe_engine()
        v = C.c_double()
        e._check(e._lib.bq_probe_launch(e._ctx, int(n), C.cast(C.byref(v), _dp)))
        return float(v.value)

    def probe_mfma_layout(self):
        e = self.probe_engine()
        out = np.empty(256)
        e._check(e._lib.bq_probe_mfma_layout(e._ctx, L.dptr(out)))
        return out.reshape(64, 4)


# bq_gp_sample's default jitter ladder, in multiples of the prior variance k(x, x)
SAMPLE_LADDER = (0.0, 1e-12, 1e-10, 1e-8, 1e-6)


class FitViews(object):
    """The stateless views of a fit that keep nothing with it and set no bit of its derived state:
    ``Fit`` inherits them.  (The table of a fit's consumers and events, tests/test_gp_fit_state.py,
    is over ``Fit``'s own methods; a view here brings its rows of that table with it in its own
    test file, which also holds that no other name lives here: tests/test_gp_marginal.py.)"""

    def marginal(self, xq, axes, mu, cov=None, want_mean=True, want_var=True, want_cov=False):
        """(mean, var, cov): the marginal of the fit, J(q) = int f(q, t) pi(q, t) dt over every
        axis but ``axes``, as a Gaussian process in q in closed form (bq_gp_marginal,
        bq_gp_marginal_box): mean and var (M,), cov (M, M), None where not wanted.  ``xq`` is
        (|S|, M), row a on axis axes[a], or (M,) for one kept axis; the measure pi on all d axes
        is (mu, cov) or a ``measures.BoxMeasure`` as in ``integral``.  J is the unnormalised
        marginal: its integral over q is ``integral``'s Z, the double integral of cov is var Z,
        and J / Z is the marginal posterior density.  var is latent and not clamped at 0.  Mean
        alone takes a fused route without a sweep.  A view: nothing is kept with the fit.
        ValueError for a ``measures.GaussianMixture`` (not built), for axes that are not distinct
        axes of the fit, none of them or all of them, for a kept coordinate that is not finite
        and for an illegal measure."""
        _marginal_no_mixture(mu)
        e = self._eng
        name, margs = self._measure(mu, cov)
        keep, xq = _marginal_points(xq, axes, self.d)
        M = xq.shape[1]
        mean = np.empty(M) if want_mean else None
        var = np.empty(M) if want_var else None
        cov_out = np.empty((M, M), order="F") if want_cov else None
        e._check(getattr(e._lib, "bq_gp_marginal" + name)(
            e._ctx, self._handle(), keep.ctypes.data_as(L._i32p), *(margs + (
                L.dptr(xq), M, L.dptr(mean), L.dptr(var), L.dptr(cov_out)))))
        return mean, var, cov_out


class Fit(FitViews):
    """Device-resident GP fit (bq_fit): L, z = L^-1 y, log-ML; alpha on demand."""

    def __init__(self, eng, x, y, h, w, s):
        self._eng = eng
        self._h = C.c_void_p()
        x = _pts(x)
        self.d, self.n = x.shape
        w = _wvec(w, self.d)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (self.n,):
            raise ValueError("y has invalid shape")
        eng._check(eng._lib.bq_gp_fit(eng._ctx, L.dptr(x), L.dptr(y), self.d, self.n, float(h),
                                      L.dptr(w), float(s), C.byref(self._h)))

    def close(self):
        if self._h is not None and self._h.value and self._eng._ctx.value:
            self._eng._lib.bq_fit_destroy(self._eng._ctx, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None or not self._h.value:
            raise ValueError("fit is closed")
        return self._h

    def refit(self, h, w, s):
        w = _wvec(w, self.d)
        e = self._eng
        e._check(e._lib.bq_gp_refit(e._ctx, self._handle(), float(h), L.dptr(w), float(s)))

    def set_y(self, y):
        """New targets for the same points; the fit must be refitted before its next use."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (self.n,):
            raise ValueError("y has invalid shape")
        e = self._eng
        e._check(e._lib.bq_gp_set_y(e._ctx, self._handle(), L.dptr(y)))

    def append(self, x_new, y_new):
        """Append k observations under the current hyper-parameters (bq_gp_append): O(k n^2) on
        the resident factor, no refactorisation.  x_new is (d, k), or (k,) for d = 1; y_new is
        (k,).  LinAlgError (the new points make the system singular) leaves the fit as it was."""
        x_new = _pts(x_new)
        if x_new.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        k = x_new.shape[1]
        y_new = np.ascontiguousarray(y_new, dtype=np.float64)
        if k < 1 or y_new.shape != (k,):
            raise ValueError("y has invalid shape")
        e = self._eng
        e._check(e._lib.bq_gp_append(e._ctx, self._handle(), L.dptr(x_new), L.dptr(y_new), k))
        self.n += k

    def remove(self, idx):
        """Remove the observations idx (distinct indices in [0, n), any order, any integer
        sequence) under the current hyper-parameters (bq_gp_remove): O(k n^2) on the resident
        factor from the first removed index on, no refactorisation; the survivors keep their
        order.  ValueError (no index, every point, out of range, a duplicate, a stale or closed
        fit) leaves the fit as it was."""
        idx = np.asarray(idx)
        if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
            raise ValueError("idx must be a non-empty one-dimensional sequence of integers")
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        e = self._eng
        e._check(e._lib.bq_gp_remove(e._ctx, self._handle(), idx.ctypes.data_as(L._i64p),
                                     idx.size))
        self.n -= idx.size

    def refit_predict(self, h, w, s, xo):
        """New hyper-parameters and the posterior mean / marginal variance at xo in one sweep
        (bq_gp_refit_predict: the hyper-parameter loop's body)."""
        w = _wvec(w, self.d)
        xo = _pts(xo)
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        M = xo.shape[1]
        mean, var = np.empty(M), np.empty(M)
        e = self._eng
        e._check(e._lib.bq_gp_refit_predict(e._ctx, self._handle(), float(h), L.dptr(w), float(s),
                                            L.dptr(xo), M, L.dptr(mean), L.dptr(var)))
        return mean, var

    @property
    def logml(self):
        v = C.c_double()
        e = self._eng
        e._check(e._lib.bq_gp_logml(e._ctx, self._handle(), C.cast(C.byref(v), _dp)))
        return float(v.value)

    def logml_grad(self):
        """Gradient of the log marginal likelihood, (d + 2,): [d/dh, d/dw_1 .. d/dw_d, d/ds]
        (bq_gp_logml_grad)."""
        g = np.empty(self.d + 2)
        e = self._eng
        e._check(e._lib.bq_gp_logml_grad(e._ctx, self._handle(), L.dptr(g)))
        return g

    def logml_hess(self):
        """Hessian of the log marginal likelihood, (d + 2, d + 2), symmetric, in the order of
        ``logml_grad``: [h, w_1 .. w_d, s] (bq_gp_logml_hess)."""
        H = np.empty((self.d + 2, self.d + 2))
        e = self._eng
        e._check(e._lib.bq_gp_logml_hess(e._ctx, self._handle(), L.dptr(H)))
        return H

    def loo(self):
        """Leave-one-out cross-validation (bq_gp_loo): (mean, var, logpred, total) -- the
        predictive mean, variance (of the noisy observation) and log density of every y_i from
        the other n - 1 observations, (n,) each, and the sum of logpred."""
        mean, var, lp = np.empty(self.n), np.empty(self.n), np.empty(self.n)
        total = C.c_double()
        e = self._eng
        e._check(e._lib.bq_gp_loo(e._ctx, self._handle(), L.dptr(mean), L.dptr(var), L.dptr(lp),
                                  C.cast(C.byref(total), _dp)))
        return mean, var, lp, float(total.value)

    def loo_grad(self):
        """(total, grad): the leave-one-out log predictive density and its gradient, (d + 2,) in
        the order of ``logml_grad`` (bq_gp_loo_grad)."""
        g = np.empty(self.d + 2)
        total = C.c_double()
        e = self._eng
        e._check(e._lib.bq_gp_loo_grad(e._ctx, self._handle(), C.cast(C.byref(total), _dp),
                                       L.dptr(g)))
        return float(total.value), g

    def lgo(self, groups):
        """Leave-group-out cross-validation (bq_gp_lgo): (mean, var, logpred, total).  ``groups``
        is a sequence of integer index sequences, disjoint, of 1 to 64 indices in [0, n) each; they
        need not cover the fit.  mean and var, (T,) in the order of the concatenated groups: the
        predictive mean and variance (of the noisy observation) of every member from the points
        outside its group; logpred, (G,): each group's joint log density at its targets; total:
        their sum.  ValueError for groups that break these rules, LinAlgError when a group's
        block of Kxx^-1 is not positive definite."""
        idx, start = _flat_groups(groups)
        T, G = idx.size, start.size - 1
        mean, var, lp = np.empty(T), np.empty(T), np.empty(G)
        total = C.c_double()
        e = self._eng
        e._check(e._lib.bq_gp_lgo(e._ctx, self._handle(), idx.ctypes.data_as(L._i64p),
                                  start.ctypes.data_as(L._i64p), G, L.dptr(mean), L.dptr(var),
                                  L.dptr(lp), C.cast(C.byref(total), _dp)))
        return mean, var, lp, float(total.value)

    def lgo_grad(self, groups):
        """(total, grad): the leave-group-out log predictive density of ``groups`` (see ``lgo``;
        the same bits as its total) and its gradient, (d + 2,) in the order of ``logml_grad``
        (bq_gp_lgo_grad)."""
        idx, start = _flat_groups(groups)
        g = np.empty(self.d + 2)
        total = C.c_double()
        e = self._eng
        e._check(e._lib.bq_gp_lgo_grad(e._ctx, self._handle(), idx.ctypes.data_as(L._i64p),
                                       start.ctypes.data_as(L._i64p), start.size - 1,
                                       C.cast(C.byref(total), _dp), L.dptr(g)))
        return float(total.value), g

    def _get(self, which, shape):
        out = np.empty(shape, order="F")
        e = self._eng
        e._check(e._lib.bq_gp_get(e._ctx, self._handle(), which, L.dptr(out)))
        return out

    def L(self):
        return self._get(0, (self.n, self.n))

    def alpha(self):
        return self._get(1, (self.n,))

    def z(self):
        return self._get(2, (self.n,))

    def K(self):
        return self._get(3, (self.n, self.n))

    def solve(self, B):
        """Kxx^-1 B with the resident factor; B is (n,) or (n, nrhs)."""
        B = np.asfortranarray(B, dtype=np.float64)
        nrhs = 1 if B.ndim == 1 else B.shape[1]
        if B.shape[0] != self.n:
            raise ValueError("b has invalid size")
        X = np.empty_like(B, order="F")
        e = self._eng
        e._check(e._lib.bq_gp_solve(e._ctx, self._handle(), L.dptr(B), nrhs, L.dptr(X)))
        return X

    def predict(self, xo, want_mean=True, want_var=True, want_cov=False):
        xo = _pts(xo)
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        M = xo.shape[1]
        mean = np.empty(M) if want_mean else None
        var = np.empty(M) if want_var else None
        cov = np.empty((M, M), order="F") if want_cov else None
        e = self._eng
        e._check(e._lib.bq_gp_predict(e._ctx, self._handle(), L.dptr(xo), M, L.dptr(mean), L.dptr(var),
                                      L.dptr(cov)))
        return mean, var, cov

    def predict_grad(self, xo, want_var=True):
        """(mean, var, dmean, dvar) at the points xo: the posterior and its gradients with
        respect to the points themselves, in closed form on the resident factor
        (bq_gp_predict_grad).  mean, var: (M,); dmean, dvar: (d, M), entry [k, j] = d/d xo[k, j].
        ``want_var=False`` leaves var and dvar None and takes the route without a sweep."""
        xo = _pts(xo)
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        M = xo.shape[1]
        mean, dmean = np.empty(M), np.empty((self.d, M), order="F")
        var = np.empty(M) if want_var else None
        dvar = np.empty((self.d, M), order="F") if want_var else None
        e = self._eng
        e._check(e._lib.bq_gp_predict_grad(e._ctx, self._handle(), L.dptr(xo), M, L.dptr(mean),
                                           L.dptr(var), L.dptr(dmean), L.dptr(dvar)))
        return mean, var, dmean, dvar

    def predict_dtheta(self, xo, want_var=True):
        """(mean, var, dmean, dvar) at the points xo: the posterior and its derivatives with
        respect to the hyper-parameters, in closed form on the resident factor
        (bq_gp_predict_dtheta).  mean, var: (M,); dmean, dvar: (d + 2, M), entry [p, j] =
        d/d theta_p at xo[:, j], theta in the order of ``logml_grad``: [h, w_1 .. w_d, s].
        ``want_var=False`` leaves var and dvar None and takes the route without a sweep."""
        xo = _pts(xo)
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        M = xo.shape[1]
        mean, dmean = np.empty(M), np.empty((self.d + 2, M), order="F")
        var = np.empty(M) if want_var else None
        dvar = np.empty((self.d + 2, M), order="F") if want_var else None
        e = self._eng
        e._check(e._lib.bq_gp_predict_dtheta(e._ctx, self._handle(), L.dptr(xo), M, L.dptr(mean),
                                             L.dptr(var), L.dptr(dmean), L.dptr(dvar)))
        return mean, var, dmean, dvar

    def _trend_key(self, degree, center, scale):
        """(degree, center, scale, p) of a trend call as the library takes them; what they may be
        is the library's to check."""
        degree = int(degree)
        center = np.ascontiguousarray(np.atleast_1d(center), dtype=np.float64).ravel()
        scale = np.ascontiguousarray(np.atleast_1d(scale), dtype=np.float64).ravel()
        if center.shape != (self.d,) or scale.shape != (self.d,):
            raise ValueError("center and scale must have d entries")
        if degree not in (0, 1, 2):
            raise ValueError("trend: degree %d, not 0 .. 2" % degree)
        p = (1, 1 + self.d, 1 + self.d + self.d * (self.d + 1) // 2)[degree]
        return degree, center, scale, p

    def trend(self, degree, center, scale):
        """(beta, cov_beta, logml_t, alpha_t): the polynomial trend of the fit with its
        coefficients marginalised under a flat prior (bq_gp_trend).  The basis over
        t = (x - center) / scale: 1; t_1 .. t_d (degree >= 1); t_k t_l, k <= l, k outer (degree
        2).  beta, (p,): the coefficients' posterior mean; cov_beta, (p, p): their covariance;
        logml_t: the log marginal likelihood with beta integrated out (its constant is that of
        the scaled basis); alpha_t, (n,): Kxx^-1 (y - H beta).  ValueError for a bad degree,
        centre or scale or fewer observations than basis functions, LinAlgError when
        H^T Kxx^-1 H is not positive definite.  The fit itself stays zero-mean."""
        degree, center, scale, p = self._trend_key(degree, center, scale)
        beta, cov, alpha = np.empty(p), np.empty((p, p), order="F"), np.empty(self.n)
        logml = C.c_double()
        e = self._eng
        e._check(e._lib.bq_gp_trend(e._ctx, self._handle(), degree, L.dptr(center), L.dptr(scale),
                                    L.dptr(beta), L.dptr(cov), C.cast(C.byref(logml), _dp),
                                    L.dptr(alpha)))
        return beta, cov, float(logml.value), alpha

    def predict_trend(self, xo, degree, center, scale, want_var=True):
        """(mean, var) of the trend posterior at the points xo (bq_gp_predict_trend; the basis as
        in ``trend``): the mean follows the trend away from the data, and var -- latent, like
        ``predict``'s -- carries the coefficients' uncertainty on top of ``predict``'s.
        ``want_var=False`` leaves var None and takes the route without a sweep."""
        xo = _pts(xo)
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        degree, center, scale, _ = self._trend_key(degree, center, scale)
        M = xo.shape[1]
        mean = np.empty(M)
        var = np.empty(M) if want_var else None
        e = self._eng
        e._check(e._lib.bq_gp_predict_trend(e._ctx, self._handle(), degree, L.dptr(center),
                                            L.dptr(scale), L.dptr(xo), M, L.dptr(mean),
                                            L.dptr(var)))
        return mean, var

    def trend_last_route(self):
        """(route, gemm_kernel) of the last ``predict_trend``: 0 the fused mean launch, 1 the
        one-pass row reductions, 2 the product (bq_gp_trend_last_route)."""
        r, k = C.c_int(), C.c_int()
        e = self._eng
        e._check(e._lib.bq_gp_trend_last_route(e._ctx, self._handle(), C.byref(r), C.byref(k)))
        return int(r.value), int(k.value)

    def sample(self, xo, S=1, z=None, seed=0, ladder=None, want_chol=False):
        """(out, mean, jitter[, chol]): S joint draws of the latent posterior at the points xo,
        on the device (bq_gp_sample).  out: (M, S) Fortran-ordered, column s one draw
        mean + L_c z_s with L_c L_c^T = cov + jitter I (no s^2, as ``predict``'s cov); mean: (M,),
        ``predict``'s bits; jitter: the absolute value added to the diagonal, k(x, x) times the
        first entry of ``ladder`` that factors (default: SAMPLE_LADDER).  z: (M, S)
        standard normals of the caller's; None: the device draws them, Philox4x32-10 keyed by the
        64-bit ``seed`` (ignored when z is given).  ``want_chol`` appends L_c, (M, M), its strict
        upper triangle zero.  LinAlgError when no ladder entry factors."""
        xo = _pts(xo)
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        M, S = xo.shape[1], int(S)
        if z is not None:
            z = np.asfortranarray(z, dtype=np.float64)
            if z.shape != (M, S):
                raise ValueError("z must be (M, S)")
        if ladder is not None:
            ladder = np.ascontiguousarray(np.atleast_1d(ladder), dtype=np.float64)
            if ladder.ndim != 1:
                raise ValueError("ladder must be a sequence of numbers")
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed must fit 64 bits")
        out, mean = np.empty((M, max(S, 0)), order="F"), np.empty(M)
        chol = np.empty((M, M), order="F") if want_chol else None
        jitter = C.c_double()
        e = self._eng
        e._check(e._lib.bq_gp_sample(e._ctx, self._handle(), L.dptr(xo), M, S, L.dptr(z), seed,
                                     L.dptr(ladder), 0 if ladder is None else ladder.size,
                                     L.dptr(out), L.dptr(mean), L.dptr(chol),
                                     C.cast(C.byref(jitter), _dp)))
        res = (out, mean, float(jitter.value))
        return res + (chol,) if want_chol else res

    def pivoted_cholesky(self, xo, q, nugget=0.0, tol=0.0, want_factor=True):
        """(piv, C, resid, gain): the greedy, diagonally pivoted partial Cholesky factorisation of
        the latent posterior covariance at the points xo, at most q steps, on the device and
        without forming the covariance (bq_gp_pivchol).  Each step takes the point with the
        largest remaining variance (the lowest index among equals): piv, (rank,) int64, is the
        max-variance sequential design; gain, (rank,), the variance each pivot had when taken;
        C, (M, rank) Fortran-ordered (None without ``want_factor``), the factor's columns
        c_j = (cov[:, p_j] - sum_{i<j} c_i c_i[p_j]) / sqrt(gain_j + nugget); resid, (M,), the
        variances left, diag(cov - C C^T).  ``nugget`` >= 0 is absolute: with s^2, resid is the
        variance after noisy observations at the pivots.  The factorisation ends early, rank < q,
        at a gain of at most ``tol`` k(x, x), or one that is not positive."""
        xo = _pts(xo)
        if xo.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        M, q = xo.shape[1], int(q)
        piv, gain = np.empty(max(q, 0), dtype=np.int64), np.empty(max(q, 0))
        fac = np.empty((M, max(q, 0)), order="F") if want_factor else None
        resid = np.empty(M)
        rank = C.c_int64()
        e = self._eng
        e._check(e._lib.bq_gp_pivchol(e._ctx, self._handle(), L.dptr(xo), M, q, float(nugget),
                                      float(tol), piv.ctypes.data_as(L._i64p), L.dptr(fac),
                                      L.dptr(resid), L.dptr(gain), C.byref(rank)))
        r = int(rank.value)
        return piv[:r], (fac[:, :r] if want_factor else None), resid, gain[:r]

    def ivr_design(self, xc, q, xr=None, rho=None, nugget=0.0, tol=0.0, want_scores=False):
        """(piv, gain, ivar0, resid_r, resid_c[, score0]): the greedy design that minimises the
        integrated posterior variance sum_j rho_j var(xr_j) by observing at most q of the
        candidates xc, on the device (bq_gp_ivr).  Each step takes the candidate whose observation
        (with noise ``nugget`` >= 0, absolute) lowers the integral the most, the lowest index
        among equals: piv, (rank,) int64; gain, (rank,), the drop each step brought; ivar0 the
        integral before the first step, so that ivar0 - gain.sum() is what is left; resid_r, (R,),
        and resid_c, (A,), the latent variances left at the reference points and at the
        candidates -- with nugget = s^2 those after ``append`` of the chosen points.  ``xr`` None:
        the candidates are the reference points (one sweep over them) and resid_r is resid_c.
        ``rho`` None: uniform weights 1 / R.  ``want_scores`` appends step 0's scores, (A,): the
        acquisition surface, 0 where a candidate is not eligible.  The run ends early, rank < q,
        at a gain of at most ``tol`` k(x, x) sum(rho), or one that is not positive."""
        xc = _pts(xc)
        if xc.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        A, q = xc.shape[1], int(q)
        if xr is not None:
            xr = _pts(xr)
            if xr.shape[0] != self.d:
                raise ValueError("dimension mismatch")
            if xr.shape[1] == 0:
                raise ValueError("no reference points")
        R = A if xr is None else xr.shape[1]
        if rho is None:
            rho = np.full(R, 1.0 / max(R, 1))
        rho = np.ascontiguousarray(rho, dtype=np.float64).ravel()
        if rho.shape[0] != R:
            raise ValueError("%d weights for %d reference points" % (rho.shape[0], R))
        piv, gain = np.empty(max(q, 0), dtype=np.int64), np.empty(max(q, 0))
        resid_c = np.empty(A)
        resid_r = None if xr is None else np.empty(R)
        score0 = np.empty(A) if want_scores else None
        ivar0, rank = C.c_double(), C.c_int64()
        e = self._eng
        e._check(e._lib.bq_gp_ivr(e._ctx, self._handle(), L.dptr(xr), 0 if xr is None else R,
                                  L.dptr(rho), L.dptr(xc), A, q, float(nugget), float(tol),
                                  piv.ctypes.data_as(L._i64p), L.dptr(gain), C.byref(ivar0),
                                  L.dptr(resid_r), L.dptr(resid_c), L.dptr(score0),
                                  C.byref(rank)))
        r = int(rank.value)
        res = (piv[:r], gain[:r], float(ivar0.value), resid_c if xr is None else resid_r, resid_c)
        return res + (score0,) if want_scores else res

    def _measure(self, mu, cov):
        """("" | "_box" | "_mix", the C arguments of the measure): (mu, cov) spell a Gaussian; a
        ``measures`` object in place of mu, with no cov, is that measure.  The returned arrays
        are referenced by the tuple, which the caller holds across the call."""
        if isinstance(mu, Measure):
            if cov is not None:
                raise TypeError("a measure object comes without a cov")
            if mu.d != self.d:
                raise ValueError("the measure has dimension %d, the fit %d" % (mu.d, self.d))
            return _measure_args(mu)
        if cov is None:
            raise TypeError("a Gaussian measure needs its cov")
        mu, cov = self._eng._mc(self.d, mu, cov)
        return "", (L.dptr(mu), L.dptr(cov))

    def integral(self, mu, cov=None, want_weights=False):
        """(mean, var[, weights]): vanilla Bayesian quadrature of the fit, the posterior mean and
        variance of Z = int f(x) N(x | mu, cov) dx (bq_gp_integral) -- or, with a
        ``measures.BoxMeasure`` or ``measures.GaussianMixture`` in place of mu and no cov, of the
        integral against that measure (bq_gp_integral_box, bq_gp_integral_mix; TypeError for a
        measure object with a cov, ValueError for one of another dimension).  var is latent, like
        ``predict``'s, and not clamped at 0.  ``want_weights`` appends the quadrature weights
        Kxx^-1 kappa_X, (n,): mean = weights . y.  The kernel means of the measure at the fit's
        points stay with the fit: a second call with the same measure is one dot product.
        ValueError for a measure that is not finite or whose covariance is not positive
        definite."""
        e = self._eng
        name, margs = self._measure(mu, cov)
        mean, var = C.c_double(), C.c_double()
        wts = np.empty(self.n) if want_weights else None
        e._check(getattr(e._lib, "bq_gp_integral" + name)(
            e._ctx, self._handle(), *(margs + (C.byref(mean), C.byref(var), L.dptr(wts)))))
        res = (float(mean.value), float(var.value))
        return res + (wts,) if want_weights else res

    def integral_design(self, xc, q, mu, cov=None, nugget=0.0, tol=0.0, want_scores=False):
        """(piv, gain, zvar0, resid_u, resid_c[, score0]): the greedy design that minimises the
        posterior variance of Z = int f(x) N(x | mu, cov) dx by observing at most q of the
        candidates xc, on the device (bq_gp_zdesign; sequential Bayesian quadrature); a
        ``measures`` object in place of mu, with no cov, as in ``integral``.  Each step
        takes the candidate whose observation (with noise ``nugget`` >= 0, absolute) lowers var Z
        the most, the lowest index among equals: piv, (rank,) int64; gain, (rank,), the drop each
        step brought; zvar0 is ``integral``'s var, so that zvar0 - gain.sum() is what is left --
        with nugget = s^2 the var after ``append`` of the chosen points; resid_u, (A,), the
        covariances of Z with the latent function at the candidates that are left and resid_c,
        (A,), the latent variances left there.  ``want_scores`` appends step 0's scores, (A,): the
        acquisition surface, 0 where a candidate is not eligible.  The run ends early, rank < q,
        at a gain of at most ``tol`` times the prior variance of Z, or one that is not positive."""
        xc = _pts(xc)
        if xc.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        e = self._eng
        name, margs = self._measure(mu, cov)
        A, q = xc.shape[1], int(q)
        piv, gain = np.empty(max(q, 0), dtype=np.int64), np.empty(max(q, 0))
        resid_u, resid_c = np.empty(A), np.empty(A)
        score0 = np.empty(A) if want_scores else None
        zvar0, rank = C.c_double(), C.c_int64()
        e._check(getattr(e._lib, "bq_gp_zdesign" + name)(
            e._ctx, self._handle(), *(margs + (
                L.dptr(xc), A, q, float(nugget), float(tol), piv.ctypes.data_as(L._i64p),
                L.dptr(gain), C.byref(zvar0), L.dptr(resid_u), L.dptr(resid_c), L.dptr(score0),
                C.byref(rank)))))
        r = int(rank.value)
        res = (piv[:r], gain[:r], float(zvar0.value), resid_u, resid_c)
        return res + (score0,) if want_scores else res

    def sq_integral(self, mu, cov, want_r=False):
        """(sq, var[, r]): square-root-warped Bayesian quadrature of the fit (WSABI-L,
        bq_gp_sqintegral).  The fit's targets are g = sqrt(2 (l - alpha0)) of an integrand
        l >= alpha0, and l = alpha0 + g^2 / 2 is linearised about the posterior mean m of g:
        sq = int m(x)^2 N(x | mu, cov) dx, so that the integral of l has mean alpha0 + sq / 2, and
        var is its variance, latent and not clamped at 0.  ``want_r`` appends r = W(X, X) alpha,
        (n,), the kernel means of the linearised integral at the fit's points (sq = alpha . r).
        The state stays with the fit per measure until its targets or its factor change.
        ValueError for a measure that is not finite or whose covariance is not positive
        definite."""
        e = self._eng
        _sq_gaussian_only(mu)
        mu, cov = e._mc(self.d, mu, cov)
        sq, var = C.c_double(), C.c_double()
        r = np.empty(self.n) if want_r else None
        e._check(e._lib.bq_gp_sqintegral(e._ctx, self._handle(), L.dptr(mu), L.dptr(cov),
                                         C.byref(sq), C.byref(var), L.dptr(r)))
        res = (float(sq.value), float(var.value))
        return res + (r,) if want_r else res

    def sq_integral_design(self, xc, q, mu, cov, nugget=0.0, tol=0.0, want_scores=False):
        """(piv, gain, zvar0, resid_u, resid_c[, score0]): ``integral_design`` for the
        square-root-warped integral of ``sq_integral`` (bq_gp_sqdesign): each step takes the
        candidate whose observation (of g, with noise ``nugget``) lowers the variance of the
        linearised integral the most with the posterior mean held at its current value.  zvar0 is
        ``sq_integral``'s var; ``tol`` is in multiples of the prior variance of that integral.
        Everything else is as in ``integral_design``."""
        xc = _pts(xc)
        if xc.shape[0] != self.d:
            raise ValueError("dimension mismatch")
        e = self._eng
        _sq_gaussian_only(mu)
        mu, cov = e._mc(self.d, mu, cov)
        A, q = xc.shape[1], int(q)
        piv, gain = np.empty(max(q, 0), dtype=np.int64), np.empty(max(q, 0))
        resid_u, resid_c = np.empty(A), np.empty(A)
        score0 = np.empty(A) if want_scores else None
        zvar0, rank = C.c_double(), C.c_int64()
        e._check(e._lib.bq_gp_sqdesign(e._ctx, self._handle(), L.dptr(mu), L.dptr(cov), L.dptr(xc),
                                       A, q, float(nugget), float(tol),
                                       piv.ctypes.data_as(L._i64p), L.dptr(gain), C.byref(zvar0),
                                       L.dptr(resid_u), L.dptr(resid_c), L.dptr(score0),
                                       C.byref(rank)))
        r = int(rank.value)
        res = (piv[:r], gain[:r], float(zvar0.value), resid_u, resid_c)
        return res + (score0,) if want_scores else res


class Pair(object):
    """GP1 over log l at the samples and GP2 over [l_s, exp(mean of GP1 at x_c)] at samples +
    candidates, evaluated at S hyper-parameter sets in one batched pass (bq_pair_*): the
    hyper-parameter objective of bq.py:536-550 and the acquisition under sampled
    hyper-parameters of bq.py:604-662."""

    def __init__(self, eng, x_s, tl_s, l_s, x_c, x_a, S):
        self._eng = eng
        self._h = C.c_void_p()
        def c(a):
            if a is None:
                return np.empty(0)
            return np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)

        x_s, tl_s, l_s, x_c, x_a = c(x_s), c(tl_s), c(l_s), c(x_c), c(x_a)
        self.ns, self.nc, self.ma, self.S = x_s.shape[0], x_c.shape[0], x_a.shape[0], int(S)
        if tl_s.shape != x_s.shape or l_s.shape != x_s.shape:
            raise ValueError("shape mismatch")
        eng._check(eng._lib.bq_pair_create(eng._ctx, L.dptr(x_s), L.dptr(tl_s), L.dptr(l_s),
                                           self.ns, L.dptr(x_c) if self.nc else None, self.nc,
                                           L.dptr(x_a) if self.ma else None, self.ma, self.S,
                                           C.byref(self._h)))

    def close(self):
        if self._h is not None and self._h.value and self._eng._ctx.value:
            self._eng._lib.bq_pair_destroy(self._eng._ctx, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _params(self, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        if p.shape != (self.S, 3):
            raise ValueError("parameters must be S x 3: (h, w, s) per set")
        return p

    def llh(self, p_tl, p_l):
        """(llh[S], l_c[S, nc], status[S]); llh = -inf where status != 0."""
        p_tl, p_l = self._params(p_tl), self._params(p_l)
        llh = np.empty(self.S)
        l_c = np.empty((self.S, self.nc))
        status = np.zeros(self.S, dtype=np.int32)
        e = self._eng
        e._check(e._lib.bq_pair_llh(e._ctx, self._h, L.dptr(p_tl), L.dptr(p_l), L.dptr(llh),
                                    L.dptr(l_c) if self.nc else None,
                                    status.ctypes.data_as(L._i32p)))
        return llh, l_c, status

    def esm(self, p_tl, p_l, thresh, mu, cov):
        """The acquisition's ingredients for every set and acquisition point: dict with A_a,
        A_sc_l, status, tm_a, tC_a (all S x ma), l_c (S x nc), sstatus (S)."""
        p_tl, p_l = self._params(p_tl), self._params(p_l)
        mu, cov = Engine._mc(1, mu, cov)
        S, ma = self.S, self.ma
        out = {k: np.empty((S, ma)) for k in ("A_a", "A_sc_l", "tm_a", "tC_a")}
        out["status"] = np.zeros((S, ma), dtype=np.int32)
        out["l_c"] = np.empty((S, self.nc))
        out["sstatus"] = np.zeros(S, dtype=np.int32)
        e = self._eng
        e._check(e._lib.bq_pair_esm(
            e._ctx, self._h, L.dptr(p_tl), L.dptr(p_l), float(thresh), L.dptr(mu), L.dptr(cov),
            L.dptr(out["A_a"]), L.dptr(out["A_sc_l"]), out["status"].ctypes.data_as(L._i32p),
            L.dptr(out["tm_a"]), L.dptr(out["tC_a"]), L.dptr(out["l_c"]) if self.nc else None,
            out["sstatus"].ctypes.data_as(L._i32p)))
        return out


class Plan(object):
    """Resident batched fit+posterior pipeline (bq_plan); what bench.py times."""

    def __init__(self, eng, nprob, d, n, M):
        self._eng = eng
        self._h = C.c_void_p()
        self.nprob, self.d, self.n, self.M = int(nprob), int(d), int(n), int(M)
        eng._check(eng._lib.bq_plan_create(eng._ctx, self.nprob, self.d, self.n, self.M,
                                           C.byref(self._h)))

    def close(self):
        if self._h is not None and self._h.value and self._eng._ctx.value:
            self._eng._lib.bq_plan_destroy(self._eng._ctx, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None or not self._h.value:
            raise ValueError("plan is closed")
        return self._h

    def nbytes(self):
        v = C.c_size_t()
        self._eng._check(self._eng._lib.bq_plan_bytes(self._handle(), C.byref(v)))
        return int(v.value)

    def check_guards(self):
        """(buffers that carry a sentinel band, sentinel bytes overwritten) -- see
        Engine.set_guard; synchronises."""
        g, bad = C.c_int64(), C.c_int64()
        self._eng._check(self._eng._lib.bq_plan_check_guards(self._eng._ctx, self._handle(),
                                                             C.byref(g), C.byref(bad)))
        return int(g.value), int(bad.value)

    def set_inputs(self, x, y, xo, h, w, s):
        """x: (P, d, n) or (P, n); y: (P, n); xo: (P, d, M) or (P, M);
        h, s: (P,) or scalars; w: (P, d), (P,) or (d,)."""
        P, d, n, M = self.nprob, self.d, self.n, self.M
        x = np.asarray(x, dtype=np.float64).reshape(P, d, n)
        xb = np.ascontiguousarray(np.transpose(x, (0, 2, 1)))
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(P, n))
        if M:
            xo = np.asarray(xo, dtype=np.float64).reshape(P, d, M)
            xob = np.ascontiguousarray(np.transpose(xo, (0, 2, 1)))
        else:
            xob = None
        h = np.ascontiguousarray(np.broadcast_to(np.asarray(h, dtype=np.float64), (P,)))
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(s, dtype=np.float64), (P,)))
        w = np.asarray(w, dtype=np.float64)
        if w.ndim <= 1 and w.size == d:
            w = np.broadcast_to(w.reshape(1, d), (P, d))
        elif w.size == P and d == 1:
            w = w.reshape(P, 1)
        elif w.size == P and d > 1:
            w = np.repeat(w.reshape(P, 1), d, axis=1)
        w = np.ascontiguousarray(w.reshape(P, d))
        e = self._eng
        e._check(e._lib.bq_plan_set_inputs(e._ctx, self._handle(), L.dptr(xb), L.dptr(y), L.dptr(xob),
                                           L.dptr(h), L.dptr(w), L.dptr(s)))

    def run(self):
        e = self._eng
        e._check(e._lib.bq_plan_run(e._ctx, self._handle()))

    def results(self):
        P, M = self.nprob, self.M
        mean, var = np.empty((P, M)), np.empty((P, M))
        logml = np.empty(P)
        status = np.zeros(P, dtype=np.int32)
        e = self._eng
        e._check(e._lib.bq_plan_results(e._ctx, self._handle(), L.dptr(mean) if M else None,
                                        L.dptr(var) if M else None, L.dptr(logml),
                                        status.ctypes.data_as(L._i32p)))
        return mean, var, logml, status


_engines = {}


def get_engine(device=None):
    """Process-wide engine for a device (default: LOCAL_RANK or 0)."""
    import os
    if device is None:
        device = int(os.environ.get("BQ_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        n = C.c_int(0)
        L.load_library().bq_device_count(C.byref(n))
        if n.value > 0:
            device %= n.value
    if device not in _engines:
        _engines[device] = Engine(device)
    return _engines[device]


def set_engine(eng, device=0):
    """Install an engine object (tests install a CPU test double here)."""
    _engines[device] = eng
