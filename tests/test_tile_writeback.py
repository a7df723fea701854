"""How the one-launch Cholesky steps (csrc/slab.h, slab_step_kernel) hand their tiles to memory.

BQ_TILE_WT (launch_config.h, tile_wt; default on): a step whose workgroups all run in one round
stores its updated tiles -- every one but workgroup 0's, which goes to the factor -- with
write-through stores, so that their write-back runs under workgroup 0's pivot chain instead of at
the launch's end.  BQ_TILE_WT=0 keeps plain stores.  Same values at the same addresses: every
context must give the same BITS, in the factor's memory and in a plan's outputs.

The last step of a sweep that carries its read-out (BQ_FOLD_READOUT, the default) no longer stores
its tiles -- slab_emit has taken what anybody reads of them -- and the workgroups of its
off-diagonal tiles without the y row return at entry (tile column 0 excepted: it stores the solved
border rows).  A tile or a store that WAS read after all shows against BQ_FOLD_READOUT=0, whose
finalize launch reads the stored Schur complement, and in a resident fit, which reads the border
rows.

Sizes: two to five launches, the smallest at which a wrong store form or a skipped tile can show.
"""
import contextlib
import os
import re

import numpy as np
import pytest

from engine_env import engine_env
from test_cholesky_contracts import EPS, fwd_err, matrix, reference
from test_slab_wave_groups import _bits, _pack, _unpack

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONTEXTS = (("default", {}), ("plain_stores", {"BQ_TILE_WT": "0"}),
            ("four_waves", {"BQ_POTF2_8W": "0"}), ("finalize", {"BQ_FOLD_READOUT": "0"}))


@pytest.fixture(scope="module")
def engines(engine):
    with contextlib.ExitStack() as stack:
        yield {name: stack.enter_context(engine_env(env, probes=True)) for name, env in CONTEXTS}


# ---- the factor's memory -------------------------------------------------------------------------
# n = 128: one step, a lone diagonal tile, stored; 192: workgroup 0's tile goes to the factor, one
# off-diagonal and one diagonal tile are stored write-through, then the last step; 320: four steps,
# tile column 0 into the scratch column, ping-pong
@gpu
@pytest.mark.parametrize("family", ["dense", "graded"])
@pytest.mark.parametrize("n", [128, 192, 320])
def test_factor_memory_same_bits_and_within_the_bound(engines, n, family):
    """The whole lower triangle and info: the same bits with write-through and with plain stores;
    e_gpu <= 4 e_ref + 64 eps against the long-double factor."""
    A = matrix(family, n, 0)
    src = _pack([A], n)
    outs = {}
    for name in ("default", "plain_stores"):
        buf = src.copy()
        info, route = engines[name].probe_potrf_batch(buf, 1, n, None, n, n * n)
        assert route[0] == "slab", (name, route)
        outs[name] = (np.tril(_unpack(buf, 0, n, n)), info)
    (Lw, iw), (Lp, ip) = outs["default"], outs["plain_stores"]
    assert np.array_equal(iw, ip) and not iw.any(), (iw, ip)
    assert np.array_equal(_bits(Lw), _bits(Lp)), (n, family)
    L_ld, e_ref = reference(family, n, 0)
    e_gpu = fwd_err(Lw, L_ld)
    print("tile write-back %s n %d e_gpu %.3e e_ref %.3e" % (family, n, e_gpu, e_ref))
    assert e_gpu <= 4 * e_ref + 64 * EPS, (n, family, e_gpu, e_ref)


# ---- plans ---------------------------------------------------------------------------------------
def _problem(B, n, M, seed):
    """test_folded_readout_matches_finalize's problems: jittered grid, sin + noise."""
    rs = np.random.RandomState(seed)
    dx = 10.0 / n
    x = np.linspace(-5, 5, n)[None, :] + 0.2 * dx * rs.uniform(-1, 1, (B, n))
    y = np.sin(x) + 0.1 * rs.randn(B, n)
    xo = rs.uniform(-5, 5, (B, max(M, 1)))[:, :M]
    return x, y, xo, 1.3, np.array([1.3 * dx]), 1e-3


def _run_guarded(eng, B, n, M, inputs, runs=1):
    """[results of every run] of a new plan under sentinel bands; no band damaged."""
    x, y, xo, h, w, s = inputs
    eng.set_guard(True)
    try:
        plan = eng.plan(B, 1, n, M)
    finally:
        eng.set_guard(False)
    try:
        plan.set_inputs(x, y, xo if M else None, h, w, s)
        res = []
        for _ in range(runs):
            plan.run()
            res.append(plan.results())
        guarded, damaged = plan.check_guards()
    finally:
        plan.close()
    assert guarded > 0 and damaged == 0, (guarded, damaged)
    return res


def _same_bits(got, want, what):
    for g, w_ in zip(got, want):
        assert g.shape == w_.shape and np.array_equal(
            np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w_).view(np.uint8)), what


PLAN_CASES = [(1, 130, 33), (1, 200, 1), (3, 200, 33), (1, 320, 64), (2, 64, 64), (5, 40, 0),
              (1, 63, 1)]


@gpu
@pytest.mark.parametrize("B,n,M", PLAN_CASES)
def test_plans_same_bits_in_every_context(engines, oracle, B, n, M):
    """mean, var, log-ML and status: the same bits in the default context, with plain stores and
    on four waves; within 1e-10 of the oracle; no sentinel band damaged."""
    inputs = _problem(B, n, M, 100 * n + M + B)
    res = {name: _run_guarded(engines[name], B, n, M, inputs)[0]
           for name in ("default", "plain_stores", "four_waves")}
    for name in ("plain_stores", "four_waves"):
        _same_bits(res[name], res["default"], (name, B, n, M))
    mean, var, logml, status = res["default"]
    assert (status == 0).all()
    x, y, xo, h, w, s = inputs
    for b in range(B):
        Lo, ao, lmo = oracle.gp_fit(x[b], y[b], h, w, s)
        assert abs(logml[b] - lmo) <= 1e-10 * abs(lmo), (b, logml[b], lmo)
        if M:
            mo, vo = oracle.gp_predict(x[b], h, w, Lo, ao, xo[b])
            assert np.max(np.abs(mean[b] - mo)) <= 1e-10 * np.max(np.abs(mo)), b
            assert np.max(np.abs(var[b] - vo)) <= 1e-10 * oracle.kernel_scale(1, h, w), b


@gpu
def test_no_skipped_tile_or_store_is_read(engines, oracle):
    """(1, 130, 33): three row blocks in the last step, the y row in the last.  The finalize
    launch of BQ_FOLD_READOUT=0 reads the stored Schur complement that the folded sweep no longer
    writes: the two agree at test_folded_readout_matches_finalize's tolerance."""
    B, n, M = 1, 130, 33
    inputs = _problem(B, n, M, 100 * n + M + B)
    mean, var, logml, status = _run_guarded(engines["default"], B, n, M, inputs)[0]
    mean0, var0, logml0, status0 = _run_guarded(engines["finalize"], B, n, M, inputs)[0]
    assert (status == 0).all() and (status0 == 0).all()
    assert np.abs(logml - logml0).max() <= 1e-13 * np.abs(logml).max()
    assert np.max(np.abs(mean - mean0)) <= 1e-13 * np.max(np.abs(mean0))
    assert np.max(np.abs(var - var0)) <= 1e-13 * oracle.kernel_scale(1, inputs[3], inputs[4])


@gpu
def test_replay_gives_the_same_bytes(engines):
    """(1, 320, 64), ten runs of one plan -- the first captures, the others replay the graph."""
    B, n, M = 1, 320, 64
    res = _run_guarded(engines["default"], B, n, M, _problem(B, n, M, 5), runs=10)
    assert (res[0][3] == 0).all()
    for rep, r in enumerate(res[1:]):
        _same_bits(r, res[0], rep + 1)


# n = 200 (npad = 256): the last diagonal block holds points 192 .. 199, the one before it 128 ..
# 191.  Eight copies of an earlier point and no noise: a pivot of each copy is rounding error, and
# the first one that is not positive fails the factor inside that block.
@gpu
@pytest.mark.parametrize("first", [192, 128])
def test_failure_same_status_and_nans(engines, first):
    """A repeated point that fails in the last diagonal block, and in the block before it: the same
    status and the same bits (NaNs included) with write-through and with plain stores."""
    B, n, M = 1, 200, 33
    x, y, xo, h, w, s = _problem(B, n, M, 9)
    x[0, first:first + 8] = x[0, 3]
    y[0, first:first + 8] = y[0, 3]
    inputs = (x, y, xo, h, w, 0.0)
    res = {name: _run_guarded(engines[name], B, n, M, inputs)[0]
           for name in ("default", "plain_stores")}
    status = res["default"][3]
    print("tile write-back failure: first copy %d status %s" % (first, status))
    assert first < status[0] <= first + 8, status
    _same_bits(res["plain_stores"], res["default"], first)


@gpu
def test_resident_fit_reads_the_border_rows(engines):
    """n = 200: z comes off the y row of the factor, which the last step's tile column 0 still
    stores: predictions at three points and log-ML, the same bits in both contexts."""
    x, y, _, h, w, s = _problem(1, 200, 1, 17)
    xo = np.array([-3.3, 0.1, 4.2])
    out = {}
    for name in ("default", "plain_stores"):
        fit = engines[name].gp_fit(x[0], y[0], h, w, s)
        try:
            mean, var, _ = fit.predict(xo)
            out[name] = (mean, var, np.array([fit.logml]))
        finally:
            fit.close()
    assert np.isfinite(out["default"][0]).all() and np.isfinite(out["default"][2]).all()
    _same_bits(out["plain_stores"], out["default"], "fit")


def test_readme_names_the_test_of_the_write_through_switch():
    """README's list of switches has BQ_TILE_WT with a test that exists in this file, and the one
    list of launch switches has it as a member that launch_slab_step reads."""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = " ".join(f.read().split())
    m = re.search(r"`BQ_TILE_WT[^`]*`[^;]*?-- `test_tile_writeback\.py::(test_\w+)`", text)
    assert m, "README has no BQ_TILE_WT line that names a test of this file"
    assert callable(globals().get(m.group(1))), m.group(1)
    with open(os.path.join(ROOT, "bayesian-quadrature_amd", "csrc", "launch_config.h")) as f:
        assert re.search(r'X\(tile_wt,\s*"BQ_TILE_WT",\s*1\)', f.read())
    with open(os.path.join(ROOT, "bayesian-quadrature_amd", "csrc", "k_panel.hip")) as f:
        assert "cfg.tile_wt" in f.read()
