"""What every kernel behind a product C -= P Q^T computes, on EXACT operands, and which kernel it is.

gemm_route (csrc/k_gemm.hip) is the one place that picks a product's kernel; launch_gemm reports the
route it ran and bq_probe_gemm_product hands it the caller's operands.  The sweeps that reach these
kernels run on banded or nearly diagonal operands almost everywhere: here each of the nine kernels,
both MFMA forms of the register-streaming ones and the fused diagonal factor get a dense product of
their own, named by the table below (computed for 256 CUs; on another CU count the failing
assertion names the case).

Operands are small integers, so the answer is exact: P and Q uniform in [-8, 8], row r of P scaled
by 2^(r // 64 % 4), C uniform in [-2^20, 2^20], k <= 512.  Every partial sum in every summation
order is an integer far below 2^53, so numpy's float64 C - P Q^T is THE result and every kernel
returns it bit for bit; a tile that reads another tile's rows is off by a factor of two.

Per case: (1) the route is the table's; (2) on or below the diagonal (everywhere without `lower`),
inside m x min(n, ccut), C is the exact result; (3) strictly above the diagonal an entry is its
input or the exact result (the kernels skip at 16-, 32- or 64-column granularity); (4) everything
else -- rows m .. ldc - 1, columns from ccut on, the k-contiguous Q's padding is never a result --
comes back bit-identical; (5) a fused launch leaves the factor of the updated leading 64 x 64 block
and its reciprocal pivots, inside the bar of test_cholesky_contracts._check_factor, or the failing
column.
"""
import contextlib

import numpy as np
import pytest

from test_cholesky_contracts import EPS, SENTINEL, _bits_equal, _engine_env, fwd_err, ld_cholesky

gpu = pytest.mark.gpu

KERNELS = ("Lds128", "Lds64", "Lds64QT", "Sub128", "Sub64", "Sub32", "K64x64", "K64x32", "SplitK")
NO_LDS = {"BQ_GEMM_LDS": "0"}


def _case(m, n, k, kernel, mfma=0, env=None, grid=None, fused=False, seeded=False,
          assemble_first=False, **opts):
    return dict(m=m, n=n, k=k, env=env or {}, opts=opts, grid=grid,
                route=dict(kernel=kernel, mfma=mfma, fused=fused, seeded=seeded,
                           assemble_first=assemble_first))


# name -> shape, options of Engine.probe_gemm_product, the route at 256 CUs
CASES = {
    "sub32_444": _case(64, 64, 32, "Sub32", 4),
    "sub32_16": _case(48, 48, 40, "Sub32", 16),
    "k64x32": _case(64, 64, 64, "K64x32"),
    "sub64_444": _case(768, 768, 40, "Sub64", 4),
    "sub64_16": _case(752, 752, 40, "Sub64", 16),
    "k64x64": _case(752, 752, 64, "K64x64"),
    "sub128_444": _case(2048, 2048, 40, "Sub128", 4),
    "sub128_16": _case(2032, 2048, 40, "Sub128", 16),
    "lds64": _case(768, 768, 64, "Lds64"),
    "lds64_tri": _case(1024, 1024, 64, "Lds64", lower=1, grid=(136, 1, 1)),
    # k < 64: no 64-tile; too few 128-tiles
    "sub64_k32": _case(768, 768, 32, "Sub64", 4),
    # the BQ_LDS_MIN_TILES fall-through
    "lds128_min_tiles": _case(1280, 1280, 32, "Lds128"),
    "lds64_batch64": _case(256, 256, 64, "Lds64", lower=1, batch=64),
    "lds128_small128": _case(256, 256, 64, "Lds128", lower=1, batch=172),
    "lds128_sharing1": _case(4096, 4096, 64, "Lds128", lower=1, sharing=1),
    "lds64_sharing2": _case(4096, 4096, 64, "Lds64", lower=1, sharing=2),
    "lds64_sharing1": _case(1024, 1024, 64, "Lds64", lower=1, sharing=1),
    "lds64qt": _case(768, 768, 64, "Lds64QT", qt=True, ldq=768),
    # an odd ldq: no 16-byte DMA
    "k64x64_odd_ldq": _case(768, 768, 64, "K64x64", qt=True, ldq=769),
    "fused_k64x32": _case(128, 64, 64, "K64x32", lower=1, want_fuse=True, fused=True),
    "fused_sub32": _case(128, 64, 32, "Sub32", 4, lower=1, want_fuse=True, fused=True),
    # a slab never gets an LDS tile
    "fused_k64x32_slab": _case(4096, 64, 64, "K64x32", lower=1, want_fuse=True, fused=True),
    "fused_k64x32_fails": _case(128, 64, 64, "K64x32", lower=1, want_fuse=True, fused=True,
                                fail_at=37),
    "not_fused_lds64": _case(1024, 1024, 64, "Lds64", lower=1, want_fuse=True),
    "fused_k64x64": _case(1024, 1024, 64, "K64x64", lower=1, want_fuse=True, fused=True,
                          env=NO_LDS),
    "fused_sub64": _case(1024, 1024, 128, "Sub64", 4, lower=1, want_fuse=True, fused=True,
                         env=NO_LDS),
    "fused_sub128": _case(2944, 2944, 128, "Sub128", 4, lower=1, want_fuse=True, fused=True,
                          env=NO_LDS),
    "tile64_768": _case(768, 768, 64, "Lds64", env={"BQ_GEMM_TILE": "64"}),
    "tile128_768": _case(768, 768, 64, "Lds128", env={"BQ_GEMM_TILE": "128"}),
    "tile64_1280": _case(1280, 1280, 64, "Lds64", env={"BQ_GEMM_TILE": "64"}),
    "tile128_1280": _case(1280, 1280, 64, "Lds128", env={"BQ_GEMM_TILE": "128"}),
    # the two forms of launch_gemm_rows
    "rows_splitk": _case(64, 256, 256, "SplitK", rows=True, grid=(2, 8, 1)),
    "rows_lds64": _case(128, 4096, 64, "Lds64", rows=True),
    "ccut": _case(1024, 1024, 64, "Lds64", lower=1, ccut=320),
}
# seeded products have no operands here (they need a problem's points): the route alone
ROUTE_ONLY = {
    "seed_d1": _case(768, 768, 64, "Lds64", seed_d=1, seeded=True),
    "seed_d2": _case(768, 768, 64, "Lds64", seed_d=2, seeded=True),
    "seed_d3": _case(768, 768, 64, "Lds64", seed_d=3, assemble_first=True),
    "seed_no_lds": _case(768, 768, 32, "Sub64", 4, seed_d=2, assemble_first=True),
    "seed_lds128": _case(1280, 1280, 32, "Lds128", seed_d=1, seeded=True),
}
J0 = 192  # global column of the fused cases' diagonal block


def _sentinel(shape):
    a = np.empty(shape, order="F")
    a.view(np.uint64)[...] = SENTINEL
    return a


def _operands(c):
    """(C, P, Q, exact) of a case, seeded from its shape: C (m + 16, n batch) with SENTINEL rows below
    row m, P packed, Q packed or (qt) k-contiguous with SENTINEL rows from k on; exact[b] = the
    m x n result of batch element b.  A fused case's updated leading block is 64 I + G G^T, G
    integer in [-2, 2] (fail_at: its diagonal entry fail_at - 1 set to -1)."""
    m, n, k, o = c["m"], c["n"], c["k"], c["opts"]
    batch, qt = o.get("batch", 1), o.get("qt", False)
    rs = np.random.RandomState((m * 1000003 + n * 10007 + k * 101 + batch) % 2 ** 32)
    scale = np.ldexp(1.0, np.arange(m) // 64 % 4)[:, None]
    P = np.asfortranarray(rs.randint(-8, 9, (m, k * batch)) * scale)
    Qm = rs.randint(-8, 9, (n, k * batch)).astype(np.float64)
    C = _sentinel((m + 16, n * batch))
    C[:m] = rs.randint(-2 ** 20, 2 ** 20 + 1, (m, n * batch))
    PQ = [P[:, b * k:(b + 1) * k] @ Qm[:, b * k:(b + 1) * k].T for b in range(batch)]
    if o.get("want_fuse"):
        G = rs.randint(-2, 3, (64, 64)).astype(np.float64)
        A = 64.0 * np.eye(64) + G @ G.T
        if o.get("fail_at"):
            A[o["fail_at"] - 1, o["fail_at"] - 1] = -1.0
        C[:64, :64] = A + PQ[0][:64, :64]
    exact = [C[:m, b * n:(b + 1) * n] - PQ[b] for b in range(batch)]
    if qt:
        Q = _sentinel((o["ldq"], n * batch))
        for b in range(batch):
            Q[:k, b * n:(b + 1) * n] = Qm[:, b * k:(b + 1) * k].T
    else:
        Q = np.asfortranarray(Qm)
    return C, P, Q, exact


@contextlib.contextmanager
def _context(engine, env):
    """The suite's engine, or one created with the case's BQ_* switches (read at creation)."""
    if not env:
        yield engine
    else:
        with _engine_env(env, probes=True) as pe:
            yield pe


def _probe(eng, c, operands=None):
    C, P, Q = operands if operands else (None, None, None)
    # (Q's leading dimension: the array's own, or named where only the route is asked for)
    o = {k: v for k, v in c["opts"].items() if k != "fail_at" and (k != "ldq" or not operands)}
    if o.get("want_fuse"):
        o["j0"] = J0
    return eng.probe_gemm_product(c["m"], c["n"], c["k"], C, P, Q, **o)


def _check_route(name, c, route):
    got = {key: route[key] for key in c["route"]}
    assert got == c["route"], (name, route)
    assert route["grid"][2] == c["opts"].get("batch", 1), (name, route)
    if c["grid"]:
        assert route["grid"] == c["grid"], (name, route)


def _check_factor(name, block, exact_block, route):
    """The fused diagonal factor against the long-double factor of the exact block: forward error
    at most 4 x that of numpy's float64 Cholesky + 64 eps, the reciprocal pivots to the same bar."""
    L_ld, info = ld_cholesky(exact_block)
    assert info == 0 and route["info"][0] == 0, (name, info, route["info"])
    L64 = np.linalg.cholesky(exact_block)
    e_gpu, e_ref = fwd_err(np.tril(block), L_ld), fwd_err(L64, L_ld)
    r_ld = 1 / np.diag(L_ld)
    d_gpu, d_ref = fwd_err(route["dinv"][0], r_ld), fwd_err(1 / np.diag(L64), r_ld)
    print("fused %-20s factor e_gpu %.3e e_ref %.3e  dinv e_gpu %.3e e_ref %.3e"
          % (name, e_gpu, e_ref, d_gpu, d_ref))
    assert e_gpu <= 4 * e_ref + 64 * EPS, (name, e_gpu, e_ref)
    assert d_gpu <= 4 * d_ref + 64 * EPS, (name, d_gpu, d_ref)


def _check_product(name, c, C0, C, exact, route):
    m, n, o = c["m"], c["n"], c["opts"]
    lower, ncol = o.get("lower", 0), min(n, o.get("ccut") or n)
    below = np.tri(m, n, dtype=bool) if lower else np.ones((m, n), dtype=bool)
    assert _bits_equal(C[m:], C0[m:]), (name, "rows below m")
    for b in range(o.get("batch", 1)):
        out, inp = C[:m, b * n:(b + 1) * n], C0[:m, b * n:(b + 1) * n]
        ok = out == exact[b]
        must = below.copy()
        must[:, ncol:] = False
        if route["fused"]:
            must[:64, :64] = False  # the factor's: _check_factor
        bad = np.argwhere(must & ~ok)
        assert bad.size == 0, (name, b, len(bad), bad[:4].tolist())
        same = out.view(np.uint64) == inp.view(np.uint64)
        assert same[:, ncol:].all(), (name, b, "columns from ccut on")
        if lower:
            bad = np.argwhere(~below & ~(ok | same))
            assert bad.size == 0, (name, b, "above the diagonal", bad[:4].tolist())
    if route["fused"] and o.get("fail_at"):
        # counted as every route counts it: 1-based, from the block's global column
        assert ld_cholesky(exact[0][:64, :64])[1] == o["fail_at"]
        assert route["info"][0] == J0 + o["fail_at"], (name, route["info"])
    elif route["fused"]:
        _check_factor(name, C[:64, :64], exact[0][:64, :64], route)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_product_is_exact_on_the_route_the_table_names(engine, name):
    c = CASES[name]
    C0, P, Q, exact = _operands(c)
    C = C0.copy(order="F")
    with _context(engine, c["env"]) as pe:
        route = _probe(pe, c, (C, P, Q))
    print("route %-20s %s" % (name, route))
    _check_route(name, c, route)
    _check_product(name, c, C0, C, exact, route)


@gpu
def test_route_table_reaches_every_kernel(engine):
    """gemm_route's answer for every row (no launch; the seeded rows have no other form): the two
    tables reach all nine kernels and both MFMA forms, and each register-streaming kernel with and
    without the fused diagonal factor."""
    seen, forms, fusing = set(), set(), set()
    for name, c in sorted({**CASES, **ROUTE_ONLY}.items()):
        with _context(engine, c["env"]) as pe:
            route = _probe(pe, c)
        print("route %-20s %s" % (name, route))
        _check_route(name, c, route)
        seen.add(route["kernel"])
        forms.add(route["mfma"])
        fusing.add((route["kernel"], route["fused"]))
    assert seen == set(KERNELS), seen
    assert forms == {0, 4, 16}, forms
    for kernel in ("Sub32", "Sub64", "Sub128", "K64x32", "K64x64"):
        assert {(kernel, True), (kernel, False)} <= fusing, (kernel, fusing)
    assert not any(f for k, f in fusing if k.startswith("Lds") or k == "SplitK"), fusing


def test_probe_gemm_product_checks_its_arguments():
    """Engine.probe_gemm_product refuses bad arguments before it touches a library (no GPU here)."""
    from bayesian_quadrature_amd import Engine
    e = Engine.__new__(Engine)
    F = lambda r, c: np.zeros((r, c), order="F")
    bad = [
        dict(m=60, n=64, k=32), dict(m=64, n=72, k=32), dict(m=64, n=64, k=12),
        dict(m=0, n=64, k=32), dict(m=64, n=64, k=32, batch=0), dict(m=64, n=64, k=32, ccut=-1),
        dict(m=64, n=64, k=32, sharing=3), dict(m=64, n=64, k=32, sharing=-1),
        dict(m=64, n=64, k=32, seed_d=4), dict(m=64, n=64, k=32, seed_d=-1),
        dict(m=48, n=64, k=32, want_fuse=True), dict(m=64, n=48, k=32, want_fuse=True),
        dict(m=64, n=64, k=64, rows=True, lower=1), dict(m=64, n=64, k=64, rows=True, batch=2),
        dict(m=64, n=64, k=64, rows=True, seed_d=1),
        # operands: all three, no seed, Fortran float64 of the right shape
        dict(m=64, n=64, k=32, C_=F(64, 64)), dict(m=64, n=64, k=32, C_=F(64, 64), P=F(64, 32)),
        dict(m=64, n=64, k=32, C_=F(64, 64), P=F(64, 32), Q=F(64, 32), seed_d=1),
        dict(m=64, n=64, k=32, C_=F(63, 64), P=F(64, 32), Q=F(64, 32)),
        dict(m=64, n=64, k=32, C_=F(64, 64), P=F(64, 40), Q=F(64, 32)),
        dict(m=64, n=64, k=32, C_=F(64, 64), P=F(64, 32), Q=F(32, 64)),
        dict(m=64, n=64, k=32, C_=F(64, 64), P=F(64, 32), Q=F(16, 64), qt=True),
        dict(m=64, n=64, k=32, C_=F(64, 64), P=F(64, 32), Q=np.zeros((64, 32))),
        dict(m=64, n=64, k=32, C_=F(64, 64), P=F(64, 32), Q=F(64, 32).astype(np.float32)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            e.probe_gemm_product(**kw)
