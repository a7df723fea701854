"""The first launch of a small system's sweep (csrc/slab.h, assemble_first_kernel): workgroup (0, 0)
computes the leading 64 x 64 block of the bordered system in the diagonal factor's registers and
factors it from there; one more workgroup takes rows 64-127 of column block 0.  BQ_FIRST_REGS=0 is
the reference: the tile stored, drained and loaded back.  Both forms run the same arithmetic on the
same operands, so everything the launch leaves in memory, and everything computed from it, is the
same BITS.

The operands are DENSE: random points in d dimensions under a kernel as wide as their cloud, with
enough noise that the Gram's condition number stays near 1e3 (checked on the host) -- on the 1-D
grids of the workloads most entries are exact zeros and a block taken from the wrong place cannot
show.
"""
import contextlib

import numpy as np
import pytest

from engine_env import engine_env
from test_slab_wave_groups import _bits

gpu = pytest.mark.gpu

# (name, environment): every form of the launch against its stored-and-reloaded counterpart
CONTEXTS = (("regs", {}), ("stored", {"BQ_FIRST_REGS": "0"}),
            ("regs4", {"BQ_POTF2_8W": "0"}),
            ("stored4", {"BQ_POTF2_8W": "0", "BQ_FIRST_REGS": "0"}))
PAIRS = (("regs", "stored"), ("regs4", "stored4"))


@pytest.fixture(scope="module")
def engines(engine):
    with contextlib.ExitStack() as stack:
        yield {name: stack.enter_context(engine_env(env, probes=True)) for name, env in CONTEXTS}


def _gram(x, h, w, s):
    """Kxx + s^2 I in float64 (the kernel of csrc/host.h, make_params)."""
    d, n = x.shape
    q = np.zeros((n, n))
    c = h * h
    for k in range(d):
        q += (x[k][:, None] - x[k][None, :]) ** 2 / (w[k] * w[k])
        c /= np.sqrt(2.0 * np.pi) * w[k]
    return c * np.exp(-0.5 * q) + s * s * np.eye(n), c


def _problem(B, d, n, M, seed, checked=None):
    """(x, y, xo, h, w, s): uniform points in [-3, 3]^d, length scale 2 (4 in eight dimensions,
    where the points lie further apart): every kernel value is far from zero.  s^2 = 1e-3 n k(0)
    bounds the condition number by 1 + lambda_max / s^2 <= 1 + 1e3; the host checks it (on the first
    `checked` problems of a large batch: the bound holds for every one)."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-3, 3, (B, d, n))
    y = np.sin(x).sum(axis=1) + 0.1 * rs.randn(B, n)
    xo = rs.uniform(-3, 3, (B, d, M))
    h, w = 1.3, np.full(d, 4.0 if d == 8 else 2.0)
    _, c = _gram(x[0], h, w, 0.0)
    s = float(np.sqrt(1e-3 * n * c))
    for b in range(B if checked is None else min(B, checked)):
        K, _ = _gram(x[b], h, w, s)
        np.linalg.cholesky(K)
        assert np.linalg.cond(K) < 1e8
        assert np.min(np.abs(K)) > 1e-9 * c  # dense: no entry underflows towards zero
    return x, y, xo, h, w, s


def _same(a, b, what):
    for key in ("A", "S0", "dinv", "info", "scal"):
        ga, gb = a[key], b[key]
        if key == "info":
            assert np.array_equal(ga, gb), (what, key, ga, gb)
        else:
            assert np.array_equal(_bits(ga), _bits(gb)), (what, key)


SIZES = (19, 63, 64, 65, 100, 129)


# ---- memory after the launch --------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d", (1, 2, 8))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: p[0])
def test_memory_state_same_bytes(engines, d, pair):
    """Everything bq_probe_first_launch returns -- the first block column of A with the leading
    block's upper triangle, the scratch column, the factor's record, info, scal; untouched bytes
    included -- under BQ_FIRST_REGS=1 against 0: npad 64 / 128 / 192, ntot from 128 (no idle tile
    in the grid) up, a border that reaches into tile (0, 0) and none (M = 0)."""
    new, old = engines[pair[0]], engines[pair[1]]
    for n in SIZES:
        for M in (0, 1, 10):
            for B in (1, 3):
                x, y, xo, h, w, s = _problem(B, d, n, M, 1000 * n + 10 * M + d + B)
                got = new.probe_first_launch(x, y, xo, h, w, s)
                want = old.probe_first_launch(x, y, xo, h, w, s)
                _same(got, want, (d, n, M, B))
                assert not got["info"].any(), (d, n, M, B, got["info"])
                # the launch wrote what it should: the leading block's factor (identity padding
                # behind n), its strict upper triangle as assembled, the rows below in A and S0
                K, c0 = _gram(x[0], h, w, s)
                m = min(n, 64)
                Kp = np.eye(64)
                Kp[:m, :m] = K[:m, :m]
                blk = got["A"][0, :64, :64]
                assert np.max(np.abs(np.tril(blk) - np.linalg.cholesky(Kp))) < 1e-10
                assert np.max(np.abs(np.triu(blk, 1) - np.triu(Kp, 1))) < 1e-13 * c0
                assert np.array_equal(_bits(got["A"][0, 64:, :]), _bits(got["S0"][0, 64:, :]))
                if n > 64:
                    k2 = min(n, 128)
                    assert np.max(np.abs(got["S0"][0, 64:k2, :] - K[64:k2, :64])) < 1e-13 * c0


@gpu
def test_memory_state_large_batch(engines):
    """Tiny systems, more of them than twice the chip's compute units: the launcher takes the
    256-thread form by its own rule (k_panel.hip, launch_assemble_d), under the default context."""
    new, old = engines["regs"], engines["stored"]
    B = 2 * new.info()["cus"] + 44  # ntot = 128: two tiles per system
    x, y, xo, h, w, s = _problem(B, 1, 19, 1, 77)
    got = new.probe_first_launch(x, y, xo, h, w, s)
    _same(got, old.probe_first_launch(x, y, xo, h, w, s), B)
    assert not got["info"].any()


# ---- every column of every wave -----------------------------------------------------------------
# column c = 4 (NW q + w) + s: with eight waves wave w owns panels w and 8 + w, with four waves
# panels w, 4 + w, 8 + w, 12 + w.  One column of every panel, s going round.
COLUMNS = tuple(4 * p + (p % 4) for p in range(16))


@gpu
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: p[0])
def test_every_column_reaches_the_factor(engines, pair):
    """n = 64, one point moved at a time: the leading factor moves -- the column's point is read
    from the right place by the wave that owns it -- and is the BQ_FIRST_REGS=0 bits."""
    new, old = engines[pair[0]], engines[pair[1]]
    x, y, xo, h, w, s = _problem(1, 2, 64, 1, 5)
    base = new.probe_first_launch(x, y, xo, h, w, s)
    for c in COLUMNS:
        xm = x.copy()
        xm[0, :, c] += 0.37
        got = new.probe_first_launch(xm, y, xo, h, w, s)
        _same(got, old.probe_first_launch(xm, y, xo, h, w, s), c)
        moved = got["A"][0, :64, :64] != base["A"][0, :64, :64]
        # column c below the diagonal (the pivot itself, k(0) + s^2 under c columns' updates, need
        # not move), row c left of it and column c above it; nothing in front of them
        assert moved[c + 1:, c].any() or (c == 63 and moved[c, c]), c
        assert c == 0 or (moved[c, :c].any() and moved[:c, c].any()), c
        assert not moved[:c, :c].any(), c


# ---- outputs ------------------------------------------------------------------------------------
PLAN_CASES = [(B, d, n, M) for d in (1, 2, 8) for n in SIZES for B in (1, 3) for M in (0, 1, 10)]


@gpu
@pytest.mark.parametrize("B,d,n,M", PLAN_CASES)
def test_plan_outputs(engines, oracle, B, d, n, M):
    """mean / var / logml / status of plans: the same bits under both settings (eight and four
    waves), problem 0 against the oracle at the parity tolerance of test_gpu_parity's plans."""
    x, y, xo, h, w, s = _problem(B, d, n, M, 100 * n + 10 * M + d)
    res = {}
    for name, eng in engines.items():
        plan = eng.plan(B, d, n, M)
        plan.set_inputs(x, y, xo if M else None, h, w, s)
        plan.run()
        res[name] = plan.results()
        plan.close()
    for a, b in PAIRS:
        for got, want in zip(res[a], res[b]):
            assert np.array_equal(_bits(got) if got.dtype == np.float64 else got,
                                  _bits(want) if want.dtype == np.float64 else want), (a, b)
    mean, var, logml, status = res["regs"]
    assert (status == 0).all()
    Lo, ao, lmo = oracle.gp_fit(x[0], y[0], h, w, s)
    assert abs(logml[0] - lmo) <= 1e-10 * max(abs(lmo), 0.5 * n * np.log(2 * np.pi))
    if M:
        mo, vo = oracle.gp_predict(x[0], h, w, Lo, ao, xo[0])
        assert np.max(np.abs(mean[0] - mo)) / np.max(np.abs(mo)) < 1e-10
        assert np.max(np.abs(var[0] - vo)) / oracle.kernel_scale(d, h, w) < 1e-10


@gpu
@pytest.mark.parametrize("B,d,n,M", [(7, 8, 900, 33), (60, 8, 450, 33), (60, 2, 450, 33)])
def test_tiles_beyond_the_first_block_column(engine, oracle, B, d, n, M):
    """The rewritten tile loop where the probe does not look: 7 x ntot = 1024 is a first launch of
    128 tiles per system; 60 x ntot = 576 sweeps diagonal block first, so assemble_kernel writes
    only the first outer block's columns (a wave's sixteen columns written or not as one) and, at
    d = 8, assemble_region_kernel the rest in front of the products.  The bits of the whole
    assembly (BQ_ASM_FUSE=0, where that differs), problem 0 against the oracle."""
    x, y, xo, h, w, s = _problem(B, d, n, M, B + n + d, checked=2)
    mean, var, logml, status = engine.batch_fit_predict(x, y, h, w, s, xo)
    assert (status == 0).all()
    with engine_env({"BQ_ASM_FUSE": "0"}, probes=True) as e2:
        m2, v2, l2, st2 = e2.batch_fit_predict(x, y, h, w, s, xo)
    assert np.array_equal(_bits(mean), _bits(m2)) and np.array_equal(_bits(var), _bits(v2))
    assert np.array_equal(_bits(logml), _bits(l2)) and np.array_equal(status, st2)
    Lo, ao, lmo = oracle.gp_fit(x[0], y[0], h, w, s)
    mo, vo = oracle.gp_predict(x[0], h, w, Lo, ao, xo[0])
    assert np.max(np.abs(mean[0] - mo)) / np.max(np.abs(mo)) < 1e-10
    assert np.max(np.abs(var[0] - vo)) / oracle.kernel_scale(d, h, w) < 1e-10
    assert abs(logml[0] - lmo) <= 1e-10 * max(abs(lmo), 0.5 * n * np.log(2 * np.pi))


@gpu
@pytest.mark.parametrize("d,n", [(1, 19), (2, 64), (2, 100), (8, 129)])
def test_resident_fit_same_bits(engines, d, n):
    """gp_fit -> L(), alpha(), logml, and a refit with new parameters: fit_factor takes the same
    first launch."""
    x, y, _, h, w, s = _problem(1, d, n, 0, 31 * n + d)
    out = {}
    for name, eng in engines.items():
        fit = eng.gp_fit(x[0], y[0], h, w, s)
        first = (fit.L(), fit.alpha(), np.array([fit.logml]))
        fit.refit(1.1 * h, 0.9 * w, 1.2 * s)
        out[name] = first + (fit.L(), fit.alpha(), np.array([fit.logml]))
        fit.close()
    for a, b in PAIRS:
        for got, want in zip(out[a], out[b]):
            assert np.array_equal(_bits(got), _bits(want)), (a, b)
    K, _ = _gram(x[0], h, w, s)
    assert np.allclose(out["regs"][0], np.linalg.cholesky(K), rtol=1e-9, atol=1e-12)


# ---- the failure report -------------------------------------------------------------------------
# Two equal points without noise make the Gram singular, not indefinite: the second one's pivot is
# k(0) - l^2 with l within an ulp of sqrt k(0) -- zero or a rounding error of either sign, and
# which is a property of k(0) alone once the pair lies far from every other point (their kernel
# values, 1e-79 k(0), vanish in the pivot's sums).  So the test takes the first output scale of a
# fixed list at which the REFERENCE form reports the pivot, and asks the same of the new form.
FAIL_SCALES = (1.3, 1.1, 0.9, 1.7, 0.7, 2.3, 1.9, 0.5, 1.5, 2.9)


@gpu
@pytest.mark.parametrize("col", (2, 61))
@pytest.mark.parametrize("n", (64, 100))
def test_failing_leading_block(engines, col, n):
    """A leading block that is not positive definite at column `col` -- one of wave 0's first
    panel, one of the last panel: info of the launch, and status / logml = -inf of a plan, are the
    same under both settings and report that column."""
    x, y, xo, _, w, _ = _problem(1, 2, n, 1, 9 + col)
    x[0, :, col - 1] = x[0, :, col] = 30.0
    ref = engines["stored"]
    h = next((v for v in FAIL_SCALES
              if ref.probe_first_launch(x, y, xo, v, w, 0.0)["info"][0] == col + 1), None)
    assert h is not None, "no scale of the list makes the duplicate's pivot non-positive"
    out = {}
    for name, eng in engines.items():
        got = eng.probe_first_launch(x, y, xo, h, w, 0.0)
        plan = eng.plan(1, 2, n, 1)
        plan.set_inputs(x, y, xo, h, w, 0.0)
        plan.run()
        mean, var, logml, status = plan.results()
        plan.close()
        print(name, "info", got["info"], "status", status, "logml", logml)
        assert got["info"][0] == col + 1, (name, got["info"])
        assert status[0] != 0 and logml[0] == -np.inf, (name, status, logml)
        out[name] = (got, status.copy(), logml.copy())
    for a, b in PAIRS:
        _same(out[a][0], out[b][0], (a, b))
        assert np.array_equal(out[a][1], out[b][1]) and np.array_equal(out[a][2], out[b][2])
    assert np.array_equal(out["regs"][1], out["regs4"][1])
