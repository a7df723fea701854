"""What every triangular sweep over a RESIDENT factor computes, on DENSE factors against long double.

The Cholesky routes are pinned in test_cholesky_contracts.py; this file pins the other half of every
solve (csrc/sweeps.hip, trsv.h, trsvflow.h, the rows_* kernels, gemm_rows, trsm_blk).  The factors
the rest of the suite hands these sweeps are nearly diagonal (rand_spd) or banded (Gaussian Grams of
sorted points): a wrong offset in a coupling far from the diagonal multiplies zeros there.  Here the
factor is the float64 Cholesky factor of a dense matrix (dense_spd, graded_spd with k = 4 and 8),
taken as EXACT data and handed to ONE sweep through bq_probe_sweep, which also reports the route
the sweep took (rows_route / rows_update in csrc/sweeps.hip decide it, the sweeps report it).

Reference: substitution in np.longdouble on that factor.  Right-hand sides: a 64-row standard-normal
base block, row r = 2^(r // 64) x base row r % 64 -- the scaling is exact in the reference and in
every kernel, so 64 long-double solves are the truth for any number of rows, and a row tile that
reads or writes another tile's rows is off by a factor of two.

Bar, per right-hand side: e = max|x - t| / max|t|, e_gpu <= 4 e_ref + 64 eps with e_ref the same
measure of LAPACK's float64 substitution on the same factor and right-hand side (the bar of
test_cholesky_contracts._check_factor: another summation order under the same bound).  The explicit
block inverses of the wide sweeps stay inside it: test_wide_inverse_emulation_meets_the_bar runs
the algorithm in numpy float64 on the CPU, so a GPU failure is a statement about the kernels.
"""
import numpy as np
import pytest

from test_cholesky_contracts import EPS, SENTINEL, _bits_equal, dense_spd, graded_spd

gpu = pytest.mark.gpu

FAMILIES = ("dense", "k4", "k8")
_FACTORS, _BASES, _TRUTH = {}, {}, {}


# ---- factors, right-hand sides, the reference -----------------------------------------------------
def factor(family, n):
    """L64 = the float64 Cholesky factor of the family's n x n matrix (cached), exact data from
    here on."""
    key = (family, n)
    if key not in _FACTORS:
        seed = 104729 + 31 * n + FAMILIES.index(family)
        A = dense_spd(n, seed) if family == "dense" else graded_spd(n, int(family[1:]), seed)
        _FACTORS[key] = np.asfortranarray(np.linalg.cholesky(A))
    return _FACTORS[key]


def base_rows(n, nb=64):
    """The nb x n standard-normal base block of the right-hand sides (cached)."""
    if (n, nb) not in _BASES:
        _BASES[(n, nb)] = np.random.RandomState(n + nb).standard_normal((nb, n))
    return _BASES[(n, nb)]


def scaled_rows(base, mrows, ldx=None):
    """(ldx, n) Fortran array: row r = 2^(r // nb) base[r % nb]; rows mrows .. ldx - 1 SENTINEL."""
    nb, n = base.shape
    X = np.empty((ldx or mrows, n), order="F")
    X.view(np.uint64)[...] = SENTINEL
    for r0 in range(0, mrows, nb):
        m = min(nb, mrows - r0)
        X[r0:r0 + m] = np.ldexp(base[:m], r0 // nb)
    return X


def ld_forward(L, Bm):
    """Bm L^-T (row r: L^-1 applied to right-hand side r), substitution in np.longdouble."""
    Ll = np.ascontiguousarray(L, dtype=np.longdouble)
    BT = np.ascontiguousarray(np.asarray(Bm).T, dtype=np.longdouble)
    XT = np.zeros_like(BT)
    for j in range(Ll.shape[0]):
        XT[j] = (BT[j] - Ll[j, :j] @ XT[:j]) / Ll[j, j]
    return XT.T


def ld_backward(L, Bm):
    """Bm L^-1 (row r: L^-T applied to right-hand side r), substitution in np.longdouble."""
    LT = np.ascontiguousarray(np.asarray(L).T, dtype=np.longdouble)
    BT = np.ascontiguousarray(np.asarray(Bm).T, dtype=np.longdouble)
    XT = np.zeros_like(BT)
    for j in range(LT.shape[0] - 1, -1, -1):
        XT[j] = (BT[j] - LT[j, j + 1:] @ XT[j + 1:]) / LT[j, j]
    return XT.T


def ld_inverse_t(L):
    """L^-T in np.longdouble (row r = unit right-hand side r through the forward sweep; the rows
    enter at their own column, so this is n^3 / 3)."""
    Ll = np.ascontiguousarray(L, dtype=np.longdouble)
    n = Ll.shape[0]
    XT = np.zeros((n, n), dtype=np.longdouble)     # XT[j, r] = (L^-1)[j, r], r <= j
    for j in range(n):
        XT[j, :j] = -(Ll[j, :j] @ XT[:j, :j]) / Ll[j, j]
        XT[j, j] = 1 / Ll[j, j]
    return XT.T


def row_err(X, T):
    """e per right-hand side (row): max|x - t| / max|t|."""
    T = np.asarray(T, dtype=np.longdouble)
    den = np.max(np.abs(T), axis=1)
    return np.asarray(np.max(np.abs(np.asarray(X).astype(np.longdouble) - T), axis=1) / den,
                      dtype=np.float64)


def truth(family, n, what, nb=64):
    """(T, e_ref) for the nb base rows, cached: T in long double, e_ref of LAPACK's float64
    substitution on the same factor and rows.  what: "forward", "backward", "both" (backward after
    forward, the solve) or "inverse" (L^-T, one unit right-hand side per row)."""
    from scipy.linalg import cho_solve, solve_triangular
    key = (family, n, what, nb)
    if key not in _TRUTH:
        L = factor(family, n)
        if what == "inverse":
            T = ld_inverse_t(L)
            R = solve_triangular(L, np.eye(n), lower=True).T
        else:
            Bm = base_rows(n, nb)
            if what == "forward":
                T = ld_forward(L, Bm)
                R = solve_triangular(L, Bm.T, lower=True).T
            elif what == "backward":
                T = ld_backward(L, Bm)
                R = solve_triangular(L, Bm.T, lower=True, trans="T").T
            else:
                T = ld_backward(L, truth(family, n, "forward", nb)[0])
                R = np.stack([cho_solve((L, True), b) for b in Bm])
        _TRUTH[key] = (T, row_err(R, T))
    return _TRUTH[key]


def check_rows(name, family, X, mrows, T, e_ref):
    """The bar on rows 0 .. mrows - 1 of X against the scaled truth; returns the worst ratio."""
    nb = T.shape[0]
    worst, worst_e, worst_ref = 0.0, 0.0, 0.0
    for r0 in range(0, mrows, nb):
        m = min(nb, mrows - r0)
        e = row_err(np.ldexp(X[r0:r0 + m], -(r0 // nb)), T[:m])
        assert np.all(np.isfinite(e)), (name, family, r0)
        k = int(np.argmax(e / e_ref[:m]))
        if e[k] / e_ref[k] > worst:
            worst, worst_e, worst_ref = e[k] / e_ref[k], e[k], e_ref[k]
        bad = np.nonzero(e > 4 * e_ref[:m] + 64 * EPS)[0]
        assert bad.size == 0, (name, family, "row", r0 + int(bad[0]), "e_gpu", e[bad[0]], "e_ref",
                               e_ref[bad[0]])
    print("parity-summary %-44s %-5s e_gpu %.3e e_ref %.3e ratio %.2f"
          % (name, family, worst_e, worst_ref, worst))
    return worst


# ---- the method itself, on the CPU -----------------------------------------------------------------
def wide_block(n):
    """csrc/host.h, wide_block: the columns of a step of the wide sweeps."""
    return min(n, 256) if n < 1024 else 512


def emulate(L, X, forward):
    """The wide sweeps' algorithm in numpy float64: per block of B columns a product with the
    explicit inverse of the diagonal block (inverted by substitution), then the update of everything
    beyond it."""
    from scipy.linalg import solve_triangular
    n = L.shape[0]
    B = wide_block(n)
    X, Y = X.copy(), np.empty_like(X)
    starts = list(range(0, n, B))
    for J in (starts if forward else reversed(starts)):
        b = min(B, n - J)
        W = solve_triangular(L[J:J + b, J:J + b], np.eye(b), lower=True)
        if forward:
            Y[:, J:J + b] = X[:, J:J + b] @ W.T
            X[:, J + b:] -= Y[:, J:J + b] @ L[J + b:, J:J + b].T
        else:
            Y[:, J:J + b] = X[:, J:J + b] @ W
            X[:, :J] -= Y[:, J:J + b] @ L[J:J + b, :J]
    return Y


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", [1152, 2112])
def test_wide_inverse_emulation_meets_the_bar(family, n):
    """The explicit-inverse sweeps (B = 512 here) in float64 on the CPU meet the bar of the GPU
    tests -- forward, backward and both -- on all three families; and on the dense family the
    long-double substitution agrees with LAPACK's to 1e-14."""
    L = factor(family, n)
    Bm = base_rows(n)
    Yf = emulate(L, Bm, True)
    for what, Y in (("forward", Yf), ("backward", emulate(L, Bm, False)),
                    ("both", emulate(L, Yf, False))):
        T, e_ref = truth(family, n, what)
        check_rows("emulation %s n=%d" % (what, n), family, Y, 64, T, e_ref)
        if family == "dense":
            assert e_ref.max() < 1e-14, (what, n, e_ref.max())


def test_long_double_reference_is_a_solve():
    """ld_forward / ld_backward / ld_inverse_t against the defining equations, small and odd-sized."""
    L = np.linalg.cholesky(dense_spd(97, 3))
    Bm = np.random.RandomState(1).standard_normal((5, 97))
    Ll = L.astype(np.longdouble)
    assert np.max(np.abs(ld_forward(L, Bm) @ Ll.T - Bm)) < 1e-17 * 97 * 10
    assert np.max(np.abs(ld_backward(L, Bm) @ Ll - Bm)) < 1e-17 * 97 * 10
    Y = ld_inverse_t(L)
    assert np.max(np.abs(Y @ Ll.T - np.eye(97))) < 1e-17 * 97 * 10
    assert np.all(np.tril(Y, -1) == 0)
    X = scaled_rows(Bm[:, :64].copy(), 12, 15)
    assert np.array_equal(X[5:10], 2 * Bm[:, :64]) and np.array_equal(X[10:12], 4 * Bm[:2, :64])
    assert (X[12:].view(np.uint64) == SENTINEL).all()


# ---- 1. the row sweeps ----------------------------------------------------------------------------
# (npad, mrows, ldl): the kind expected forward and backward on a device of 256 compute units --
# a small system's backward sweep has no one-launch steps, it goes out as gemm_rows products --
# and, for fused sweeps, the (LDS-tile, split-k) update steps forward and backward.
ROW_CASES = {
    (64, 64, 0): ("step", "gemm_rows", None, None),
    (320, 64, 0): ("step", "gemm_rows", None, None),        # B = 256, partial last block of 64
    (960, 128, 0): ("step", "gemm_rows", None, None),       # B = 256, partial last block of 192
    (1024, 64, 0): ("step", "gemm_rows", None, None),       # B = 512, ldl = npad + 64
    (1088, 256, 0): ("step", "gemm_rows", None, None),      # step 0 carries block 1's product
    (2112, 128, 0): ("step", "gemm_rows", None, None),
    (2112, 192, 0): ("step", "gemm_rows", None, None),
    (2112, 256, 0): ("fused", "fused", (0, 3), (2, 1)),
    (2112, 512, 0): ("fused", "fused", (1, 2), (3, 0)),
    (1152, 1152, 0): ("fused", "fused", (0, 1), (1, 0)),
}
# The fall-back.  Whole 64-row tiles with an odd ldl reach it in both directions.  96 rows reach it
# backward only: forward, rows_route hands every multiple of 32 rows that fits 4 x CUs split-k
# tiles to the one-launch steps (96 rows would need npad >= 10944 to leave them); 544 rows at
# npad = 2112 are the smallest such case that does not fit, and reach it forward.
FALLBACK_CASES = {
    (2112, 96, 0): ("step", "gemm_rows", None, None),
    (1152, 1152, 1153): ("gemm_rows", "gemm_rows", None, None),
    (2112, 544, 0): ("gemm_rows", None, None, None),
}
GRADED_TOO = ((1088, 256, 0), (2112, 512, 0))
WHICH = {"forward": "forward_rows", "backward": "backward_rows"}


def _run_rows(engine, direction, family, npad, mrows, ldl, ldx=None):
    X = scaled_rows(base_rows(npad), mrows, ldx)
    route = engine.probe_sweep(WHICH.get(direction, direction), factor(family, npad), X, mrows, ldl)
    return X, route


def _check_route(case, direction, route, table):
    fwd, bwd, fforms, bforms = table[case]
    kind, forms = (fwd, fforms) if direction == "forward" else (bwd, bforms)
    assert route["kind"] == kind, (case, direction, route)
    assert route["B"] == wide_block(case[0]), (case, route)
    assert (route["lds"], route["splitk"]) == (forms or (0, 0)), (case, direction, route)


def _row_params(table, graded=()):
    out = []
    for case in sorted(table):
        for direction in ("forward", "backward"):
            if table[case][direction == "backward"] is None:
                continue
            for family in FAMILIES if case in graded else ("dense",):
                out.append(pytest.param(direction, case, family,
                                        id="%s-%dx%d-ldl%d-%s" % ((direction,) + case + (family,))))
    return out


@gpu
@pytest.mark.parametrize("direction,case,family", _row_params(ROW_CASES, GRADED_TOO))
def test_row_sweeps_against_long_double(engine, direction, case, family):
    """enqueue_forward_rows / enqueue_backward_rows on a dense factor: the route the table names,
    every right-hand side inside the bar."""
    npad, mrows, ldl = case
    X, route = _run_rows(engine, direction, family, npad, mrows, ldl)
    _check_route(case, direction, route, ROW_CASES)
    T, e_ref = truth(family, npad, direction)
    check_rows("%s_rows %dx%d %s" % (direction, npad, mrows, route["kind"]), family, X, mrows, T,
               e_ref)


@gpu
@pytest.mark.parametrize("direction,case,family", _row_params(FALLBACK_CASES))
def test_row_sweeps_fall_back_to_gemm_rows(engine, direction, case, family):
    """The gemm_rows products: rows that are no whole 64-row tiles, and an odd leading dimension
    of the factor (which no entry point produces: pick_ld is even)."""
    npad, mrows, ldl = case
    X, route = _run_rows(engine, direction, family, npad, mrows, ldl)
    _check_route(case, direction, route, FALLBACK_CASES)
    T, e_ref = truth(family, npad, direction)
    check_rows("%s_rows %dx%d ldl=%d %s" % (direction, npad, mrows, ldl, route["kind"]), family, X,
               mrows, T, e_ref)


@gpu
def test_row_route_table_reaches_every_kind(engine):
    """Over the two tables every kind of rows_route and both update forms of a fused step are
    reached in both directions on this device; a case that another CU count moves to another route
    is named by the assertion."""
    kinds, forms = set(), set()
    before = engine.probe_engine().stats()["flow_fallbacks"]
    for table in (ROW_CASES, FALLBACK_CASES):
        for case in sorted(table):
            npad, mrows, ldl = case
            for direction in ("forward", "backward"):
                if table[case][direction == "backward"] is None:
                    continue
                _, route = _run_rows(engine, direction, "dense", npad, mrows, ldl)
                print("route %-8s %4d x %4d ldl %4d -> %s" % (direction, npad, mrows, ldl, route))
                _check_route(case, direction, route, table)
                kinds.add((direction, route["kind"]))
                if route["lds"]:
                    forms.add((direction, "lds"))
                if route["splitk"]:
                    forms.add((direction, "splitk"))
                assert route["flow_fallbacks"] == before
    assert kinds == {("forward", "step"), ("forward", "fused"), ("forward", "gemm_rows"),
                     ("backward", "fused"), ("backward", "gemm_rows")}, kinds
    assert forms == {(d, f) for d in ("forward", "backward") for f in ("lds", "splitk")}, forms


# ---- 2. the 64-column sweep and the triangular inverse ------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ["dense", "k8"])
@pytest.mark.parametrize("npad,mrows", [(64, 64), (320, 128), (1088, 64)])
def test_forward_rows_blk_against_long_double(engine, npad, mrows, family):
    """enqueue_forward_rows_blk (append, esm_border): 64 columns per step from the 16 x 16
    inverses, in place."""
    X, route = _run_rows(engine, "forward_rows_blk", family, npad, mrows, 0)
    assert route["kind"] == "blk" and route["B"] == 64, route
    T, e_ref = truth(family, npad, "forward")
    check_rows("forward_rows_blk %dx%d" % (npad, mrows), family, X, mrows, T, e_ref)


@gpu
@pytest.mark.parametrize("npad", [320, 1088])
def test_inverse_rows_against_long_double(engine, npad):
    """enqueue_inverse_rows (the gradient's Y = L^-T): the triangle bq_gp_logml_grad reads --
    Y[r, j], j >= r -- against the long-double inverse, one unit right-hand side per row; the
    strict lower triangle is not the sweep's to write."""
    Y = np.empty((npad, npad), order="F")
    Y.view(np.uint64)[...] = SENTINEL
    route = engine.probe_sweep("inverse_rows", factor("dense", npad), Y)
    assert route["kind"] == "fused" and route["B"] == wide_block(npad), route
    assert np.all(np.tril(Y, -1) == 0)
    T, e_ref = truth("dense", npad, "inverse")
    e = row_err(np.triu(Y), T)
    k = int(np.argmax(e / e_ref))
    print("parity-summary %-44s %-5s e_gpu %.3e e_ref %.3e ratio %.2f"
          % ("inverse_rows %d" % npad, "dense", e[k], e_ref[k], e[k] / e_ref[k]))
    bad = np.nonzero(~(e <= 4 * e_ref + 64 * EPS))[0]
    assert bad.size == 0, (npad, "row", int(bad[0]), e[bad[0]], e_ref[bad[0]])


# ---- 3. the single-vector sweeps ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ["dense", "k8"])
@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("npad", [64, 320, 1088, 2048, 2112, 2496])
def test_vec_sweeps_against_long_double(engine, npad, direction, family):
    """One right-hand side, one launch per block column (trsv.h), against long double; from 2048
    rows the one-launch form (trsvflow.h) returns the same bits and no hand-off times out."""
    L = factor(family, npad)
    x0 = np.asfortranarray(base_rows(npad, 1))
    X = x0.copy(order="F")
    before = engine.probe_engine().stats()["flow_fallbacks"]
    route = engine.probe_sweep(direction + "_vec", L, X)
    assert route["kind"] == "vec_block" and route["B"] == wide_block(npad), route
    T, e_ref = truth(family, npad, direction, 1)
    check_rows("%s_vec %d" % (direction, npad), family, X, 1, T, e_ref)
    if npad >= 2048:
        Xf = x0.copy(order="F")
        route = engine.probe_sweep(direction + "_vec_flow", L, Xf)
        assert route["kind"] == "vec_flow" and route["flow_fallbacks"] == before, route
        assert _bits_equal(Xf, X)
    else:
        with pytest.raises(ValueError, match="no one-launch"):
            engine.probe_sweep(direction + "_vec_flow", L, x0.copy(order="F"))


# ---- 4. strides -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which,npad,mrows", [("forward", 1088, 256), ("backward", 1088, 256),
                                              ("forward_rows_blk", 320, 128)])
def test_row_sweeps_respect_ldx(engine, which, npad, mrows):
    """ldx = mrows + 64 with the padding rows full of NaN: the result rows are the packed run's bit
    for bit, the padding rows come back bit for bit."""
    Xp, route_p = _run_rows(engine, which, "dense", npad, mrows, 0)
    X, route = _run_rows(engine, which, "dense", npad, mrows, 0, mrows + 64)
    assert route == route_p
    assert (X[mrows:].view(np.uint64) == SENTINEL).all()
    assert _bits_equal(X[:mrows], Xp)
    assert np.all(np.isfinite(Xp))


# ---- 5. bad arguments ---------------------------------------------------------------------------------
@gpu
def test_probe_sweep_bad_arguments(engine):
    from bayesian_quadrature_amd import _lib as L_
    pe = engine.probe_engine()
    n = 128
    Lm = np.asfortranarray(np.eye(n))
    X = np.asfortranarray(np.ones((96, n)))
    route = np.zeros(5, dtype=np.int32)
    rp = route.ctypes.data_as(L_._i32p)

    def call(which, n_, ldl, mrows, ldx, Lp=L_.dptr(Lm), Xp=L_.dptr(X), r=rp):
        return pe._lib.bq_probe_sweep(pe._ctx, which, n_, Lp, ldl, mrows, ldx, Xp, r)
    assert call(0, n, 0, 64, 96) == L_.BQ_OK
    assert route[0] == 0 and route[1] == 128 and np.all(X[:64] == 1) and np.all(X[64:] == 1)
    assert call(4, n, 0, 1, 96) == L_.BQ_OK and route[0] == 4
    bad = [(0, 100, 0, 64, 96), (0, 0, 0, 64, 96), (0, n, n - 1, 64, 96), (0, n, 0, 48, 96),
           (0, n, 0, 0, 96), (1, n, 0, 96, 64), (2, n, 0, 40, 96), (3, n, 0, 64, 96),
           (3, n, 0, 96, 96), (4, n, 0, 32, 96), (5, n, 0, 2, 96), (6, n, 0, 1, 96),
           (7, n, 0, 1, 96), (8, n, 0, 64, 96), (-1, n, 0, 64, 96)]
    for args in bad:
        assert call(*args) == L_.BQ_ERR_BAD_ARG, args
        assert pe._lib.bq_last_error(pe._ctx).startswith(b"sweep: "), args
    assert call(0, n, 0, 64, 96, Lp=None) == L_.BQ_ERR_BAD_ARG
    assert call(0, n, 0, 64, 96, Xp=None) == L_.BQ_ERR_BAD_ARG
    assert call(0, n, 0, 64, 96, r=None) == L_.BQ_ERR_BAD_ARG
    assert pe._lib.bq_probe_sweep(None, 0, n, L_.dptr(Lm), 0, 64, 96, L_.dptr(X), rp) == \
        L_.BQ_ERR_BAD_ARG
    # and a clean call afterwards
    assert call(1, n, 0, 96, 96) == L_.BQ_OK and route[0] == 2


# ---- 6. bq_cho_solve on the same factors ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ["dense", "k8"])
@pytest.mark.parametrize("nrhs", [1, 2, 65, 256])
@pytest.mark.parametrize("n", [1100, 2100])
def test_cho_solve_on_dense_factors(engine, n, nrhs, family):
    """bq_cho_solve with n no multiple of 64 (padding, the transposition in and out, the partial
    last block): truth is backward after forward in long double, e_ref scipy's cho_solve column by
    column."""
    L = factor(family, n)
    before = engine.stats()["flow_fallbacks"]
    B = np.asfortranarray(scaled_rows(base_rows(n), nrhs).T)     # n x nrhs, column c one solve
    Xs = np.empty((n, nrhs), order="F")
    Xs.view(np.uint64)[...] = SENTINEL
    engine.cho_solve(L, B, Xs, nrhs)
    T, e_ref = truth(family, n, "both")
    check_rows("cho_solve n=%d nrhs=%d" % (n, nrhs), family, np.ascontiguousarray(Xs.T), nrhs, T,
               e_ref)
    assert engine.stats()["flow_fallbacks"] == before
