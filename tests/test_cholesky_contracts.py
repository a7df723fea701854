"""What the C ABI promises of every Cholesky route, on DENSE input: the failing column (exactly), the
factor against a long-double reference, and leading dimensions / strides beyond the packed minimum.

The sweep has four routes (csrc/potrf.hip, sweep_route) and at least eight places that compute a
failing column, each with its own offset; a Gaussian Gram's breakdown column depends on rounding and
pins none of them.  Here the failures are PLANTED in dense, well-conditioned matrices, so the column
is known: bq_cho_factor (all three transports of the flag), bq_potrf_dev (recursive panels, the
fused diagonal factor, the look-ahead, the slab tail) and -- through bq_probe_potrf_batch, which
hands a batched route the caller's own matrices -- the one-launch steps, the blocked sweep, the two
half-batches and the diagonal-block-first sweep with both of its diagonal factors.

Reference: a plain column-by-column Cholesky in np.longdouble (ld_cholesky).  LAPACK cannot be the
only one: OpenBLAS's dpotrf returns info = 0 for a NaN on or below the diagonal.

Pivot rule of the engine: a pivot that is not a positive FINITE number fails (+inf fails too, where
LAPACK would carry on).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from engine_env import engine_env as _engine_env

gpu = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# a quiet NaN with a payload: whatever reads a padding double poisons its result, whatever writes
# one changes these bits
SENTINEL = np.uint64(0x7FF8DEADBEEF1234)


# ---- the reference ----------------------------------------------------------------------------
def ld_cholesky(A):
    """(L, info) of the lower triangle of A, column by column in np.longdouble: info is the first
    1-based column whose pivot is not a positive finite number (L then holds the columns before
    it), else 0."""
    Al = np.tril(np.asarray(A)).astype(np.longdouble)
    n = Al.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        col = Al[j:, j] - L[j:, :j] @ L[j, :j]
        p = col[0]
        if not (p > 0 and np.isfinite(p)):
            return L, j + 1
        d = np.sqrt(p)
        L[j, j] = d
        L[j + 1:, j] = col[1:] / d
    return L, 0


def ld_info_resumed(L0, A0, A, c):
    """ld_cholesky(A)'s info for a matrix A whose lower triangle differs from A0's only in rows
    >= c (checked), given A0's long-double factor L0: the rows before c of the factor are L0's,
    row c is recomputed as the plain algorithm computes it, and its pivot decides.  (A full run
    per planted column of a 4480 x 4480 matrix would take an hour.)"""
    assert np.array_equal(np.tril(A[:c, :c]), np.tril(A0[:c, :c]))
    row = np.zeros(c, dtype=np.longdouble)
    a = A[c, :c + 1].astype(np.longdouble)
    for k in range(c):
        row[k] = (a[k] - row[:k] @ L0[k, :k]) / L0[k, k]
    p = a[c] - row @ row
    if not (p > 0 and np.isfinite(p)):
        return c + 1
    raise AssertionError("the planted failure at column %d does not fail in the reference" % c)


def dense_spd(n, seed):
    """A0 = G G^T / (n + 8) + I, G an n x (n + 8) standard normal: dense, condition ~ 5."""
    rs = np.random.RandomState(seed)
    G = rs.standard_normal((n, n + 8))
    A = G @ G.T / (n + 8) + np.eye(n)
    return np.asfortranarray(0.5 * (A + A.T))


def graded_spd(n, k, seed):
    """Q diag(logspace(0, -k, n)) Q^T: condition 10^k, stands in for the small length scales."""
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    A = (Q * np.logspace(0, -k, n)) @ Q.T
    return np.asfortranarray(0.5 * (A + A.T))


_MATS, _REFS = {}, {}


def matrix(family, n, idx):
    """Matrix `idx` of a family at size n (cached): "dense", or "graded" (k = 4 for even idx, 8 for
    odd)."""
    key = (family, n, idx)
    if key not in _MATS:
        seed = 7919 * n + idx
        _MATS[key] = dense_spd(n, seed) if family == "dense" else \
            graded_spd(n, 4 if idx % 2 == 0 else 8, seed)
    return _MATS[key]


def reference(family, n, idx):
    """(long-double factor, e_ref) of matrix(family, n, idx), cached; e_ref = the forward error of
    LAPACK's fp64 dpotrf against it, max|L64 - L| / max|L|."""
    key = (family, n, idx)
    if key not in _REFS:
        from scipy.linalg import lapack
        A = matrix(family, n, idx)
        L, info = ld_cholesky(A)
        assert info == 0
        L64, i64 = lapack.dpotrf(A, lower=1)
        assert i64 == 0
        _REFS[key] = (L, fwd_err(np.tril(L64), L))
    return _REFS[key]


def fwd_err(X, X_ld):
    return float(np.max(np.abs(X.astype(np.longdouble) - X_ld)) / np.max(np.abs(X_ld)))


def bwd_err(A, L, S=None):
    """||L L^T (+ [0, 0; 0, S]) - A||_F / ||A||_F over the lower triangle; L is n x ncols."""
    R = L @ L.T
    if S is not None:
        nc = L.shape[1]
        R[nc:, nc:] += S
    R = np.tril(R - A)
    return float(np.linalg.norm(R) / np.linalg.norm(np.tril(A)))


# ---- planted failures -------------------------------------------------------------------------
NEG, NAN_DIAG, NAN_OFF, INF_DIAG = "neg", "nan_diag", "nan_off", "inf_diag"


def plant(A, c, kind):
    """Plants a failure at column c of the symmetric matrix A (in place, lower triangle; the diagonal
    is its own mirror) and returns the entries it overwrote, for restore()."""
    if kind == NAN_OFF:
        j = c // 2
        assert j < c
        old = [(c, j, A[c, j])]
        A[c, j] = np.nan
        return old
    old = [(c, c, A[c, c])]
    A[c, c] = {NEG: -5.0, NAN_DIAG: np.nan, INF_DIAG: np.inf}[kind]
    return old


def restore(A, old):
    for i, j, v in reversed(old):
        A[i, j] = v


def kinds_for(c, k):
    """Every column gets the negative pivot; the NaN kinds alternate over the column list (all of
    them where a matrix is small enough for it to cost nothing)."""
    out = [NEG, NAN_DIAG if k % 2 == 0 else NAN_OFF]
    return [kd for kd in out if not (kd == NAN_OFF and c == 0)]


def column_classes(nelim, nbs, extra=()):
    """Columns relative to the blocking: the edges of the first 64-column steps, of the outer
    blocks nb in nbs (the first four, where a blocked sweep hands over to its slab tail or leaves
    the look-ahead), the middle of the second outer block, and the last eliminated column."""
    cols = {0, 1, 62, 63, 64, 65, nelim - 2, nelim - 1, nelim // 2, nelim - 64, nelim - 65}
    for nb in nbs:
        for m in (1, 2, 3, 4):
            cols |= {m * nb - 1, m * nb, m * nb + 1}
        cols.add(nb + nb // 2)
    cols |= set(extra)
    return sorted(c for c in cols if 0 <= c < nelim)


# ---- the reference's own test (CPU) ---------------------------------------------------------------
def test_reference_cholesky_against_lapack():
    """The long-double reference reports LAPACK's column for every planted negative pivot, its
    resumed form reports the same as a full run, it sees the NaN and +inf pivots, and on clean
    matrices it is numpy's factor."""
    from scipy.linalg import lapack
    for n in (64, 192, 448, 1100):
        A0 = dense_spd(n, n)
        L0, info = ld_cholesky(A0)
        assert info == 0
        Lnp = np.linalg.cholesky(A0)
        assert fwd_err(Lnp, L0) < 1e-14
        assert bwd_err(A0, np.float64(L0)) < 1e-15
        cols = [c for c in (0, 1, 62, 63, 64, 65, 127, 128, n // 2, n - 2, n - 1) if c < n]
        for k, c in enumerate(cols):
            A = A0.copy()
            plant(A, c, NEG)
            _, i64 = lapack.dpotrf(A, lower=1)
            assert i64 == c + 1
            assert ld_info_resumed(L0, A0, A, c) == c + 1
            if n <= 448 or k % 5 == 0:
                assert ld_cholesky(A)[1] == c + 1
            if n <= 192:
                for kind in (NAN_DIAG, NAN_OFF, INF_DIAG):
                    if kind == NAN_OFF and c == 0:
                        continue
                    B = A0.copy()
                    plant(B, c, kind)
                    assert ld_cholesky(B)[1] == c + 1, (n, c, kind)
                    assert ld_info_resumed(L0, A0, B, c) == c + 1
    for k in (4, 8):
        A0 = graded_spd(320, k, k)
        L0, info = ld_cholesky(A0)
        assert info == 0
        assert fwd_err(np.linalg.cholesky(A0), L0) < 10.0 ** k * 1e-15
    # two failures: the first one
    A = dense_spd(192, 5)
    plant(A, 70, NEG)
    plant(A, 130, NAN_DIAG)
    assert ld_cholesky(A)[1] == 71


# ---- 1. bq_cho_factor through the raw ABI -----------------------------------------------------------
def _cho_factor_raw(eng, A, in_place, want_info=True):
    from bayesian_quadrature_amd import _lib as L_
    n = A.shape[0]
    Cm = np.asfortranarray(A.copy())
    Lm = Cm if in_place else np.zeros((n, n), order="F")
    info = C.c_int64(-7)
    st = eng._lib.bq_cho_factor(eng._ctx, L_.dptr(Cm), L_.dptr(Lm), n,
                                C.byref(info) if want_info else None)
    return st, info.value, Lm


@gpu
@pytest.mark.parametrize("n", [1, 2, 37, 64, 65, 100, 181, 182, 300, 1100, 3200])
def test_cho_factor_reports_the_failing_column(engine, n):
    """bq_cho_factor's *info, all three transports of the flag (n <= 64: four bytes of a staging
    double; n^2 + 1 <= 32768: a double through launch_mat_out; larger: a copy of the device int)
    and, at 3200, one matrix on the blocked route: the planted column exactly, out of place and in
    place; a clean call on the same context afterwards is BQ_OK with info 0 and the right factor;
    info = NULL is accepted."""
    from bayesian_quadrature_amd import _lib as L_
    A0 = matrix("dense", n, 0)
    L0, _ = reference("dense", n, 0)
    cols = column_classes(n, (128, 384))
    A = A0.copy()
    for k, c in enumerate(cols):
        kinds = kinds_for(c, k) if n > 1100 else \
            [kd for kd in (NEG, NAN_DIAG, NAN_OFF) if not (kd == NAN_OFF and c == 0)]
        for kind in kinds:
            old = plant(A, c, kind)
            ref = ld_info_resumed(L0, A0, A, c)
            for in_place in ((False, True) if n <= 1100 else (bool(k % 2),)):
                st, info, _ = _cho_factor_raw(engine, A, in_place)
                assert (st, info) == (L_.BQ_ERR_NOT_PD, ref), (n, c, kind, in_place, st, info)
            restore(A, old)
    assert np.array_equal(A, A0)
    # +inf on the diagonal fails at its column (the engine's pivot rule)
    c = cols[len(cols) // 2]
    old = plant(A, c, INF_DIAG)
    st, info, _ = _cho_factor_raw(engine, A, False)
    assert (st, info) == (L_.BQ_ERR_NOT_PD, c + 1)
    restore(A, old)
    # two failures: the first is reported
    if n >= 2:
        c1, c2 = cols[len(cols) // 3], cols[-1]
        assert c1 < c2
        old = plant(A, c1, NEG) + plant(A, c2, NAN_DIAG)
        st, info, _ = _cho_factor_raw(engine, A, True)
        assert (st, info) == (L_.BQ_ERR_NOT_PD, ld_info_resumed(L0, A0, A, c1))
        # info = NULL
        st, _, _ = _cho_factor_raw(engine, A, False, want_info=False)
        assert st == L_.BQ_ERR_NOT_PD
        restore(A, old)
    # and a clean call afterwards
    for in_place in (False, True):
        st, info, Lm = _cho_factor_raw(engine, A0, in_place)
        assert (st, info) == (L_.BQ_OK, 0)
        assert fwd_err(np.tril(Lm), L0) < 1e-13
        assert bwd_err(A0, np.tril(Lm)) < 1e-14 * max(n, 64)
        assert np.array_equal(np.triu(Lm, 1), np.triu(A0, 1))
    st, _, Lm = _cho_factor_raw(engine, A0, False, want_info=False)
    assert st == L_.BQ_OK and fwd_err(np.tril(Lm), L0) < 1e-13


# ---- 2. bq_potrf_dev on device-resident matrices ------------------------------------------------------
POTRF_CONFIGS = {
    "shipped": ({}, 0, True),
    "nb64": ({}, 64, True),
    "nb128": ({}, 128, True),
    "nb192": ({}, 192, True),
    "no_lookahead": ({}, 0, False),
    "la_min0": ({"BQ_LA_MIN": "0"}, 0, True),
}


class _DevMatrix(object):
    """An n x n matrix of leading dimension lda on the device, its int32 flag beside it."""

    def __init__(self, eng, n, lda):
        self.eng, self.n, self.lda = eng, n, lda
        self.A = eng.alloc(8 * lda * n)
        self.info = eng.alloc(64)

    def potrf(self, host):
        """host: the lda x n column-major buffer as a flat array; returns (status, info)."""
        e = self.eng
        assert host.ndim == 1 or host.flags.f_contiguous
        e.upload(self.A, host)
        st = e._lib.bq_potrf_dev(e._ctx, self.A, self.n, self.lda, self.info)
        hinfo = np.full(1, -7, dtype=np.int32)
        e.download(hinfo, self.info)
        return st, int(hinfo[0])

    def download(self):
        out = np.empty(self.lda * self.n)
        self.eng.download(out, self.A)
        return out

    def close(self):
        self.eng.free(self.A), self.eng.free(self.info)


@gpu
@pytest.mark.parametrize("config", sorted(POTRF_CONFIGS))
@pytest.mark.parametrize("n", [64, 448, 1152, 3072, 4480])
def test_potrf_dev_reports_the_failing_column(engine, n, config):
    """info_dev[0] of bq_potrf_dev: one-launch steps below 3072 rows, from there outer blocks of 384
    with the look-ahead and the slab tail; under bq_set_block the recursive panels with the
    diagonal factor fused into the products, without the second stream, and with the look-ahead
    kept to the last panel.  bq_potrf_dev itself returns BQ_OK: the flag is the report."""
    env, nb, la = POTRF_CONFIGS[config]
    A0 = matrix("dense", n, 0)
    L0, _ = reference("dense", n, 0)
    cols = column_classes(n, (128, 192, 384))
    with contextlib.ExitStack() as stack:
        eng = stack.enter_context(_engine_env(env)) if env else engine
        dev = _DevMatrix(eng, n, n)
        try:
            eng.set_block(nb)
            eng.set_lookahead(la)
            A = A0.copy(order="F")
            for k, c in enumerate(cols):
                kinds = kinds_for(c, k) if n > 1152 else \
                    [kd for kd in (NEG, NAN_DIAG, NAN_OFF) if not (kd == NAN_OFF and c == 0)]
                for kind in kinds:
                    old = plant(A, c, kind)
                    st, info = dev.potrf(A)
                    assert st == 0 and info == ld_info_resumed(L0, A0, A, c), \
                        (n, config, c, kind, st, info)
                    restore(A, old)
            c = cols[len(cols) // 2]
            old = plant(A, c, INF_DIAG)
            assert dev.potrf(A) == (0, c + 1)
            restore(A, old)
            if n > 64:
                c1, c2 = cols[len(cols) // 3], cols[-1]
                old = plant(A, c1, NAN_DIAG) + plant(A, c2, NEG)
                assert dev.potrf(A) == (0, c1 + 1)
                restore(A, old)
            # a clean call on the same context afterwards
            assert np.array_equal(A, A0)
            assert dev.potrf(A) == (0, 0)
            Lf = np.tril(dev.download().reshape(n, n).T)
            assert bwd_err(A0, Lf) < 1e-14 * max(n, 64)
            assert fwd_err(Lf, L0) < 1e-12
        finally:
            eng.set_block(0)
            eng.set_lookahead(True)
            dev.close()


# ---- 3. the batched routes, through bq_probe_potrf_batch ----------------------------------------------
# name: (environment, batch, ntot, the route expected, DiagFirst's diagonal factors: "wg" one
# workgroup per matrix, "steps" the one-launch steps, "both" the steps and -- for the blocks with
# df_wg_rows rows below them -- the workgroups).  The route is asserted, not assumed.
ROUTES = {
    "slab": ({}, 5, 1024, "slab", None),
    "blocked": ({}, 2, 3072, "blocked", None),
    "dfirst": ({}, 12, 1280, "diag_first", "both"),
    "dfirst_wg": ({}, 100, 704, "diag_first", "wg"),
    "halves": ({"BQ_DIAG_FIRST": "0"}, 12, 1280, "halves", None),
    "dfirst_force_wg": ({"BQ_DF_WG": "1"}, 12, 1280, "diag_first", "wg"),
    "dfirst_force_steps": ({"BQ_DF_WG": "0"}, 12, 1280, "diag_first", "steps"),
    "dfirst_rec_solve": ({"BQ_DF_SWEEP": "0"}, 12, 1280, "diag_first", "both"),
    "dfirst_late_fork": ({"BQ_DF_EARLY": "0"}, 12, 1280, "diag_first", "both"),
}
# the cases whose launches differ in more than a switch: strides and partial elimination run on them
BASE_ROUTES = ("slab", "blocked", "dfirst", "dfirst_wg", "halves")


class Batch(object):
    """`batch` matrices of a family in one flat buffer of leading dimension lda and matrix stride
    astride (0: a plan's own), padding rows and gaps filled with SENTINEL."""

    def __init__(self, eng, family, batch, ntot, lda=0, astride=0):
        self.batch, self.ntot = batch, ntot
        self.lda = lda if lda else eng.plan_ld(ntot)
        self.astride = astride if astride else self.lda * ntot
        self.lda_arg, self.astride_arg = lda, astride
        self.family = family
        self.buf = np.empty(self.astride * batch)
        self.buf.view(np.uint64)[:] = SENTINEL
        for b in range(batch):
            self.rows(self.buf, b)[:, :ntot] = matrix(family, ntot, b).T

    def rows(self, buf, b):
        """Matrix b's storage as (column, row) -- [:, :ntot] the matrix transposed, [:, ntot:] its
        padding rows."""
        o = b * self.astride
        return buf[o:o + self.lda * self.ntot].reshape(self.ntot, self.lda)

    def mat(self, buf, b):
        return self.rows(buf, b)[:, :self.ntot].T

    def outside(self, buf):
        """The bits of every double that belongs to no matrix."""
        u = buf.view(np.uint64)
        parts = []
        for b in range(self.batch):
            parts.append(self.rows(u, b)[:, self.ntot:].ravel())
            parts.append(u[b * self.astride + self.lda * self.ntot:(b + 1) * self.astride])
        return np.concatenate(parts)

    def run(self, eng, buf, ncols=None):
        info, route = eng.probe_potrf_batch(buf, self.batch, self.ntot, ncols, self.lda_arg,
                                            self.astride_arg)
        return info, route


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                          np.ascontiguousarray(b).view(np.uint64))


def _check_route(name, route):
    env, batch, ntot, kind, _ = ROUTES[name]
    assert route[0] == kind, (name, route)
    assert route[1] in (64, 128, 192, 256, 320, 384, 448, 512) and route[1] <= ntot, (name, route)
    if kind in ("slab", "diag_first") or (kind == "blocked" and batch <= 2):
        assert route[2], (name, route)


def _sample(batch):
    """The matrices compared with the long-double factor where a batch is large: both ends and
    both sides of the middle (the seam of two half-batches)."""
    return sorted({0, 1, batch // 2 - 1, batch // 2, batch - 1} & set(range(batch)))


@gpu
def test_route_table_reaches_every_sweep(engine):
    """The table above reaches all four kinds of sweep_route and both of DiagFirst's diagonal
    factors (a clean batch through each case; the probe reports the route it ran)."""
    seen, forms = set(), set()
    for name, (env, batch, ntot, kind, form) in sorted(ROUTES.items()):
        with _engine_env(env, probes=True) as pe:
            bt = Batch(pe, "dense", batch, ntot)
            buf = bt.buf.copy()
            info, route = bt.run(pe, buf)
        assert not info.any(), (name, info)
        _check_route(name, route)
        print("route %-20s %3d x %4d -> %s, nb %d" % (name, batch, ntot, route[0], route[1]))
        seen.add(route[0])
        if route[0] == "diag_first":
            # (csrc/potrf.hip, dfirst_wg and enqueue_potrf_dfirst's `diag`)
            sw = env.get("BQ_DF_WG")
            wg = batch >= 96 if sw is None else sw != "0"
            mixed = not wg and sw is None and ntot - 2 * route[1] >= 1000
            assert form == ("wg" if wg else "both" if mixed else "steps"), (name, form)
            forms |= {"wg"} if wg else {"steps", "wg"} if mixed else {"steps"}
    # one 3200-row matrix, as test_cho_factor_reports_the_failing_column pads 3200 columns to
    buf = np.ascontiguousarray(np.eye(3200)).ravel()
    info, route = engine.probe_potrf_batch(buf, 1, 3200, 3200, 3200, 3200 * 3200)
    assert info[0] == 0 and route == ("blocked", 384, True), route
    assert seen == {"slab", "blocked", "halves", "diag_first"}
    assert forms == {"wg", "steps"}
    assert {ROUTES[k][4] for k in ROUTES} >= {"wg", "steps", "both"}


@gpu
@pytest.mark.parametrize("name", sorted(ROUTES))
def test_batched_routes_report_the_failing_column(engine, name):
    """Planted failures in a batch: about a third of the matrices stay clean, the others fail at
    DIFFERENT columns on both halves of the batch; info is the reference's column for each, and
    the clean matrices' factors are the bits of a run with nothing planted (the launches and their
    data are the same)."""
    env, batch, ntot, kind, _ = ROUTES[name]
    with _engine_env(env, probes=True) as pe:
        bt = Batch(pe, "dense", batch, ntot)
        clean = bt.buf.copy()
        info, route = bt.run(pe, clean)
        assert not info.any()
        _check_route(name, route)
        nb = route[1]
        cols = column_classes(ntot, (nb,))
        # (kind by kind, so that the matrices of one run fail at different columns)
        cases = []
        for kind_ in (NEG, NAN_DIAG, NAN_OFF):
            for k, c in enumerate(cols):
                if not (kind_ == NAN_OFF and c == 0) and (batch >= 12 or kind_ in kinds_for(c, k)):
                    cases.append(((c, kind_),))
        cases.append(((cols[len(cols) // 2], INF_DIAG),))
        cases.append(((cols[len(cols) // 3], NEG), (cols[-1], NAN_DIAG)))       # two: the first
        cases.append(((cols[2], NAN_OFF), (cols[len(cols) // 2], NEG)))
        # which matrices fail: in a round r, matrix b stays clean when (b + r) % 3 == 0
        todo, rnd = list(cases), 0
        halves_hit, neighbours = set(), 0
        while todo:
            failing = [b for b in range(batch) if (b + rnd) % 3 != 0]
            if batch == 2:
                failing = [[0], [1], [0, 1]][rnd % 3]
            planted = {}
            buf = bt.buf.copy()
            for b in failing:
                if not todo:
                    break
                case = todo.pop(0)
                A0 = matrix("dense", ntot, b)
                A = A0.copy()
                for c, kind_ in case:
                    plant(A, c, kind_)
                bt.rows(buf, b)[:, :ntot] = A.T
                c_first = min(c for c, _ in case)
                planted[b] = (case, ld_info_resumed(reference("dense", ntot, b)[0], A0, A, c_first))
            info, route2 = bt.run(pe, buf)
            assert route2 == route
            for b in range(batch):
                if b in planted:
                    assert info[b] == planted[b][1], (name, rnd, b, planted[b], info[b])
                    halves_hit.add(b >= batch // 2)
                else:
                    assert info[b] == 0, (name, rnd, b, info[b])
                    assert _bits_equal(buf[b * bt.astride:(b + 1) * bt.astride],
                                       clean[b * bt.astride:(b + 1) * bt.astride]), (name, rnd, b)
                    neighbours += (b - 1 in planted) or (b + 1 in planted)
            assert len({v[1] for v in planted.values()}) >= min(len(planted), len(cols)) // 2 + \
                (len(planted) > 1), (name, rnd, planted)
            rnd += 1
        assert halves_hit == {False, True}
        assert neighbours > 0


# ---- 4. status of the points APIs: consistency ----------------------------------------------------------
@gpu
def test_plan_status_is_a_column_of_the_gram(engine):
    """The points APIs cannot take a planted matrix: for a hopeless problem status lies in [1, n]
    -- not in the identity padding, not in the border --, and the GPU does not report a column
    later than one where the long-double pivot of the Gram is already below -n eps max|K|."""
    from bayesian_quadrature_amd import workloads as wl
    P, n, M = 4, 200, 10
    rs = np.random.RandomState(0)
    dx = 10.0 / (n - 1)
    x = np.linspace(-5, 5, n)[None, :] + rs.uniform(-dx / 4, dx / 4, (P, n))
    y = wl.norm_logpdf(x)
    xo = np.tile(np.linspace(-4, 4, M), (P, 1))
    w = np.full(P, dx)
    w[2] = 50 * dx               # numerically singular Gaussian Gram, no noise
    plan = engine.plan(P, 1, n, M)
    plan.set_inputs(x, y, xo, 1.0, w, 0.0)
    plan.run()
    status = plan.results()[3]
    plan.close()
    assert (np.delete(status, 2) == 0).all()
    # (bq_batch_fit_predict shares its hyper-parameters: all four problems are hopeless)
    status2 = engine.batch_fit_predict(x, y, 1.0, np.array([w[2]]), 0.0, xo)[3]
    for p, st in [(2, status[2])] + list(enumerate(status2)):
        assert 1 <= st <= n, (p, st)
        K = engine.gram(x[p], 1.0, np.array([w[2]]), 0.0)
        thr = n * EPS * np.max(np.abs(K))
        m = int(st) - 1
        L, info = ld_cholesky(K[:m, :m])
        if info:
            j = info - 1
            pivot = np.longdouble(K[j, j]) - L[j, :j] @ L[j, :j]
            assert pivot >= -thr, (p, st, info, float(pivot), thr)


# ---- 5. - 7. the factor on dense input -----------------------------------------------------------------
def _check_factor(name, bt, buf, info, ncols, family):
    """Matrix by matrix: the backward error of everything the sweep left (every matrix), L11, L21
    and the Schur complement against the long-double reference (a sample of a large batch)."""
    ntot = bt.ntot
    worst = 0.0
    assert not info.any(), (name, info)
    for b in range(bt.batch):
        A = matrix(family, ntot, b)
        F = np.tril(bt.mat(buf, b))
        Lp = F[:, :ncols]
        S = F[ncols:, ncols:] if ncols < ntot else None
        be = bwd_err(A, Lp, S)
        assert be < 1e-14 * max(ntot, 64), (name, family, b, be)
        if b not in _sample(bt.batch):
            continue
        from scipy.linalg import lapack
        L_ld, e_full = reference(family, ntot, b)
        L64 = np.tril(lapack.dpotrf(A, lower=1)[0])
        blocks = [("L11", Lp[:ncols], L_ld[:ncols, :ncols], L64[:ncols, :ncols])]
        if ncols < ntot:
            L21 = L_ld[ncols:, :ncols]
            S_ld = np.tril(A[ncols:, ncols:].astype(np.longdouble) - L21 @ L21.T)
            S64 = np.tril(A[ncols:, ncols:] - L64[ncols:, :ncols] @ L64[ncols:, :ncols].T)
            blocks += [("L21", Lp[ncols:], L21, L64[ncols:, :ncols]), ("S", S, S_ld, S64)]
        for what, X, X_ld, X64 in blocks:
            e_gpu, e_ref = fwd_err(X, X_ld), fwd_err(X64, X_ld)
            print("parity %-18s %-6s b=%-3d ncols=%-4d %-3s e_gpu %.3e e_ref %.3e ratio %.2f"
                  % (name, family, b, ncols, what, e_gpu, e_ref, e_gpu / e_ref))
            worst = max(worst, e_gpu / e_ref)
            assert e_gpu <= 4 * e_ref + 64 * EPS, (name, family, b, what, e_gpu, e_ref)
    return worst


@gpu
@pytest.mark.parametrize("family", ["dense", "graded"])
@pytest.mark.parametrize("name", sorted(ROUTES))
def test_batched_factor_against_long_double(engine, name, family):
    """Full elimination on every route: tril(L) against the long-double factor.  Backward error
    below 1e-14 max(n, 64) (the bar of test_gp_fit); forward error at most 4 x that of LAPACK's
    fp64 dpotrf on the same matrix + 64 eps (another summation order under the same c n eps cond
    bound).  Dense A0 and the graded family (condition 1e4 in even, 1e8 in odd matrices)."""
    env, batch, ntot, kind, _ = ROUTES[name]
    with _engine_env(env, probes=True) as pe:
        bt = Batch(pe, family, batch, ntot)
        buf = bt.buf.copy()
        info, route = bt.run(pe, buf)
    _check_route(name, route)
    assert _bits_equal(bt.outside(buf), bt.outside(bt.buf))
    worst = _check_factor(name, bt, buf, info, ntot, family)
    print("parity-summary %-18s %-6s %s nb %d worst e_gpu / e_ref %.2f"
          % (name, family, route[0], route[1], worst))


@gpu
@pytest.mark.parametrize("name,borders", [("slab", (64, 128, 256)), ("blocked", (128,)),
                                          ("dfirst", (256,)), ("dfirst_wg", (64,)),
                                          ("halves", (128,)), ("dfirst_rec_solve", (64,)),
                                          ("dfirst_late_fork", (256,))])
def test_partial_elimination_against_long_double(engine, name, borders):
    """ncols < ntot with the border sizes plans use: L11, L21 = A21 L11^-T and the lower triangle of
    the Schur complement A22 - L21 L21^T, same bars."""
    env, batch, ntot, kind, _ = ROUTES[name]
    with _engine_env(env, probes=True) as pe:
        for border in borders:
            bt = Batch(pe, "dense", batch, ntot)
            buf = bt.buf.copy()
            info, route = bt.run(pe, buf, ntot - border)
            assert route[0] == kind, (name, border, route)
            assert _bits_equal(bt.outside(buf), bt.outside(bt.buf))
            worst = _check_factor(name, bt, buf, info, ntot - border, "dense")
            print("parity-summary %-18s border %d %s nb %d worst e_gpu / e_ref %.2f"
                  % (name, border, route[0], route[1], worst))


# ---- 8. leading dimensions and strides ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", BASE_ROUTES)
def test_batched_routes_respect_strides(engine, name):
    """lda = ntot + 2 and ntot + 64, astride = lda ntot + 128: the padding rows and the gaps
    between the matrices come back bit for bit, and the factor is the packed run's, bit for bit."""
    env, batch, ntot, kind, _ = ROUTES[name]
    with _engine_env(env, probes=True) as pe:
        packed = Batch(pe, "dense", batch, ntot, ntot, ntot * ntot)
        pbuf = packed.buf.copy()
        info, route = packed.run(pe, pbuf)
        assert not info.any() and route[0] == kind
        for lda, gap in ((ntot + 2, 0), (ntot + 64, 0), (ntot + 2, 128), (ntot + 64, 128)):
            bt = Batch(pe, "dense", batch, ntot, lda, lda * ntot + gap)
            buf = bt.buf.copy()
            info, route2 = bt.run(pe, buf)
            assert not info.any() and route2 == route, (name, lda, gap, route2)
            assert _bits_equal(bt.outside(buf), bt.outside(bt.buf)), (name, lda, gap)
            assert (bt.outside(buf) == SENTINEL).all()
            for b in range(batch):
                assert _bits_equal(np.tril(bt.mat(buf, b)), np.tril(packed.mat(pbuf, b))), \
                    (name, lda, gap, b)


@gpu
def test_probe_potrf_batch_bad_arguments(engine):
    from bayesian_quadrature_amd import _lib as L_
    pe = engine.probe_engine()
    buf = np.zeros(4 * 200 * 200)
    info = np.zeros(4, dtype=np.int32)
    route = np.zeros(3, dtype=np.int32)

    def call(batch, ntot, ncols, lda, astride):
        return pe._lib.bq_probe_potrf_batch(pe._ctx, batch, ntot, ncols, lda, astride,
                                            L_.dptr(buf), info.ctypes.data_as(L_._i32p),
                                            route.ctypes.data_as(L_._i32p))
    for b in range(2):
        buf[b * 128 * 128:(b + 1) * 128 * 128] = np.eye(128).ravel()
    assert call(2, 128, 128, 128, 128 * 128) == L_.BQ_OK
    assert not info.any() and route[0] == 0 and route[1] == 64
    assert np.array_equal(buf[:128 * 128].reshape(128, 128), np.eye(128))
    for args in ((2, 100, 64, 0, 0), (2, 128, 100, 0, 0), (2, 128, 192, 0, 0), (2, 128, 0, 0, 0),
                 (0, 128, 128, 0, 0), (2, 128, 128, 127, 0), (2, 128, 128, 126, 0),
                 (2, 128, 128, 129, 0), (2, 128, 128, 130, 128 * 128)):
        assert call(*args) == L_.BQ_ERR_BAD_ARG, args


@gpu
@pytest.mark.parametrize("n", [448, 1152])
def test_potrf_dev_respects_lda(engine, n):
    """bq_potrf_dev(lda > n): rows n .. lda - 1 keep their bits and the factor is the packed
    call's; an odd lda or lda < n is BQ_ERR_BAD_ARG."""
    from bayesian_quadrature_amd import _lib as L_
    A0 = matrix("dense", n, 0)
    dev = _DevMatrix(engine, n, n)
    try:
        assert dev.potrf(A0) == (0, 0)
        Lp = np.tril(dev.download().reshape(n, n).T)
        for lda in (n + 1, n - 2, n - 1):
            assert engine._lib.bq_potrf_dev(engine._ctx, dev.A, n, lda, dev.info) == \
                L_.BQ_ERR_BAD_ARG, lda
    finally:
        dev.close()
    for lda in (n + 2, n + 64):
        dev = _DevMatrix(engine, n, lda)
        try:
            host = np.empty(lda * n)
            host.view(np.uint64)[:] = SENTINEL
            R = host.reshape(n, lda)
            R[:, :n] = A0.T
            assert dev.potrf(host) == (0, 0)
            out = dev.download().reshape(n, lda)
            assert (out[:, n:].view(np.uint64) == SENTINEL).all(), lda
            assert _bits_equal(np.tril(out[:, :n].T), Lp), lda
            # and a failing column with the padding in place
            A = A0.copy()
            plant(A, n - 3, NEG)
            R[:, :n] = A.T
            assert dev.potrf(host) == (0, n - 2)
            assert (dev.download().reshape(n, lda)[:, n:].view(np.uint64) == SENTINEL).all()
        finally:
            dev.close()


@gpu
@pytest.mark.parametrize("n,d", [(100, 1), (448, 1), (1000, 2)])
def test_gram_gauss_dev_respects_ldk(engine, n, d):
    """bq_gram_gauss_dev(ldk > n): rows n .. ldk - 1 keep their bits and K is the packed call's;
    ldk < n is BQ_ERR_BAD_ARG."""
    from bayesian_quadrature_amd import _lib as L_
    rs = np.random.RandomState(n)
    x = np.ascontiguousarray(rs.uniform(-3, 3, (n, d)))       # d x n column-major
    w = np.full(d, 0.7)
    lib, ctx = engine._lib, engine._ctx
    xd = engine.alloc(8 * n * d)
    engine.upload(xd, x)
    outs = {}
    try:
        for ldk in (n, n + 2, n + 64):
            Kd = engine.alloc(8 * ldk * n)
            try:
                host = np.empty(ldk * n)
                host.view(np.uint64)[:] = SENTINEL
                engine.upload(Kd, host)
                engine._check(lib.bq_gram_gauss_dev(ctx, xd, d, n, 1.3, L_.dptr(w), 0.05, Kd, ldk))
                engine.download(host, Kd)
                R = host.reshape(n, ldk)
                assert (R[:, n:].view(np.uint64) == SENTINEL).all(), ldk
                outs[ldk] = R[:, :n].T.copy()
                if ldk == n:
                    assert lib.bq_gram_gauss_dev(ctx, xd, d, n, 1.3, L_.dptr(w), 0.05, Kd,
                                                 n - 1) == L_.BQ_ERR_BAD_ARG
            finally:
                engine.free(Kd)
    finally:
        engine.free(xd)
    K = outs[n]
    assert np.array_equal(K, engine.gram(x.T, 1.3, w, 0.05))
    for ldk in (n + 2, n + 64):
        assert _bits_equal(outs[ldk], K), ldk
