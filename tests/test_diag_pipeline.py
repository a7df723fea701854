"""A diagonal tile of the 512-thread one-launch Cholesky step (csrc/slab.h, slab_step_kernel<., 8,
true>): waves 0-3 publish every 16-column block x_c of the solved rows behind a barrier of its own
and waves 4-7 run k-block c of the tile's update while x_{c+1} is being solved; waves 4-7 then hand
the tile to the factor (workgroup 0) or store it and emit the read-out (every other diagonal tile,
the last step).  BQ_DIAG_PIPE=0 is the one-phase form (solve, barrier, update on waves 0-3) and
BQ_POTF2_8W=0 the four-wave form: the same MFMAs on the same operands in the same order per
accumulator, so every context must give the same BITS.  What can go wrong is a k-block skipped,
applied twice, read from the wrong rows or read before it was published, a block stored by the wrong
wave, and a barrier count that differs between the wave groups (a hang, not a wrong value).

The operands are DENSE (conftest.rand_spd; random points under a wide kernel), as in
test_step_loads.py: on the 1-D Gram of the workloads most of a tile is exact zeros.
"""
import contextlib
import os
import re

import numpy as np
import pytest

from engine_env import engine_env
from test_cholesky_contracts import EPS, fwd_err, ld_cholesky
from test_slab_wave_groups import _bits, _matrix, _pack, _unpack
from test_step_loads import _dense_problem

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONTEXTS = (("default", {}), ("one_phase", {"BQ_DIAG_PIPE": "0"}),
            ("four_waves", {"BQ_POTF2_8W": "0"}))


@pytest.fixture(scope="module")
def engines(engine):
    with contextlib.ExitStack() as stack:
        yield [(name, stack.enter_context(engine_env(env, probes=True))) for name, env in CONTEXTS]


def _factor(eng, name, src, batch, ntot, ld):
    buf = src.copy()
    info, route = eng.probe_potrf_batch(buf, batch, ntot, None, ld, ld * ntot)
    assert route[0] == "slab", (name, route)
    return buf, info


def _factor_all(engines, src, batch, ntot, ld, cols=None):
    """probe_potrf_batch of `src` in every context: the default context's buffer and info, after
    asserting that info and the lower triangles (columns < cols) are the same bits everywhere."""
    outs = [_factor(eng, name, src, batch, ntot, ld) for name, eng in engines]
    for (name, _), (buf, info) in zip(engines[1:], outs[1:]):
        assert np.array_equal(info, outs[0][1]), (name, info, outs[0][1])
        for b in range(batch):
            got = np.tril(_unpack(buf, b, ntot, ld))[:, :cols]
            want = np.tril(_unpack(outs[0][0], b, ntot, ld))[:, :cols]
            assert np.array_equal(_bits(got), _bits(want)), (name, ntot, b)
    return outs[0]


def _check_bound(L_gpu, L_ld, e_ref, what):
    """The bound of test_cholesky_contracts: e_gpu <= 4 e_ref + 64 eps against the long-double
    column Cholesky, e_ref = the forward error of an fp64 reference on the same matrix."""
    e_gpu = fwd_err(L_gpu, L_ld)
    print("diag pipe %s e_gpu %.3e e_ref %.3e" % (what, e_gpu, e_ref))
    assert e_gpu <= 4 * e_ref + 64 * EPS, (what, e_gpu, e_ref)


# ntot = 128: one step, one workgroup, a lone diagonal tile that goes back to memory; 192: workgroup
# 0 hands its tile to the factor and a second diagonal tile is stored; 256, 320: ping-pong steps
@gpu
@pytest.mark.parametrize("batch,pad", [(1, 0), (3, 0), (3, 8)])
@pytest.mark.parametrize("ntot", [128, 192, 256, 320])
def test_sweep_same_bits_in_every_context(engines, ntot, batch, pad):
    ld = ntot + pad
    mats = [_matrix(ntot, b) for b in range(batch)]
    out, info = _factor_all(engines, _pack([m[0] for m in mats], ld), batch, ntot, ld)
    assert not info.any(), info
    for b, (_, L, e_ref) in enumerate(mats):
        _check_bound(np.tril(_unpack(out, b, ntot, ld)), L, e_ref,
                     "ntot %d batch %d ld %d b %d" % (ntot, batch, ld, b))


_BASE = {}


def _base192(engines):
    if not _BASE:
        out, info = _factor_all(engines, _pack([_matrix(192, 0)[0]], 192), 1, 192, 192)
        assert not info.any()
        _BASE["L"] = np.tril(_unpack(out, 0, 192, 192)).copy()
    return _BASE["L"]


@gpu
@pytest.mark.parametrize("rb", range(4))
@pytest.mark.parametrize("c", range(4))
def test_every_k_block_counts_once(engines, c, rb):
    """One entry of the first panel moved, in column block c and in 16-row block rb of row block
    1: x_c of those rows moves, and with it -- through k-block c of the update -- the diagonal
    block at 64.  A k-block skipped, applied twice or read from the wrong rows leaves the bound."""
    A0 = _matrix(192, 0)[0]
    base = _base192(engines)
    A = A0.copy(order="F")
    i, k = 64 + 16 * rb + 9, 16 * c + 5
    A[i, k] += 0.375
    A[k, i] = A[i, k]
    out, info = _factor_all(engines, _pack([A], 192), 1, 192, 192)
    assert not info.any()
    Lg = np.tril(_unpack(out, 0, 192, 192))
    assert Lg[i, i] != base[i, i] and (Lg[64:128, 64:128] != base[64:128, 64:128]).any(), (c, rb)
    L_ld, linfo = ld_cholesky(A)
    assert linfo == 0
    _check_bound(Lg, L_ld, fwd_err(np.linalg.cholesky(A), L_ld),
                 "k-block %d, rows 16 x %d of row block 1" % (c, rb))


@gpu
@pytest.mark.parametrize("ntot", [192, 320])
def test_no_k_block_is_read_before_it_is_published(engines, ntot):
    """Ten factors in the default context: a k-block read in front of its barrier would take
    what the previous step left in the Q rows, now and then.  The same bits every time, and the
    four-wave factor's."""
    src = _pack([_matrix(ntot, 0)[0]], ntot)
    (name4, eng4), (name, eng) = engines[2], engines[0]
    assert name4 == "four_waves" and name == "default"
    want, info4 = _factor(eng4, name4, src, 1, ntot, ntot)
    assert not info4.any()
    for rep in range(10):
        got, info = _factor(eng, name, src, 1, ntot, ntot)
        assert not info.any()
        assert np.array_equal(_bits(np.tril(_unpack(got, 0, ntot, ntot))),
                              _bits(np.tril(_unpack(want, 0, ntot, ntot)))), (ntot, rep)


@gpu
@pytest.mark.parametrize("ntot,col", [(192, 101), (256, 76), (320, 127)])
def test_failure_report_same_in_every_context(engines, ntot, col):
    """A matrix made indefinite at a column inside the second diagonal block -- the one workgroup
    0 updates on waves 4-7 and factors: the same info (the column, 1-based) and the same bits in
    the columns in front of it."""
    A = _matrix(ntot, 0)[0].copy(order="F")
    A[col, col] = -5.0
    out, info = _factor_all(engines, _pack([A], ntot), 1, ntot, ntot, cols=col)
    assert info[0] == col + 1, info


PLAN_CASES = [(B, d, n, M) for B in (1, 3) for d in (1, 2)
              for n, M in ((64, 1), (100, 10), (130, 70), (192, 130))]


# last steps of one diagonal tile (a border of at most 64 rows) and of two diagonal tiles plus one
# off-diagonal tile (a border of up to 128 rows), with the y row in either diagonal tile
@gpu
@pytest.mark.parametrize("B,d,n,M", PLAN_CASES)
def test_read_out_from_waves_4_to_7(engines, oracle, B, d, n, M):
    """The bordered plan: the last step's diagonal tiles are stored, and mean / var / log-ML
    emitted, by waves 4-7.  The same bits in every context and on a graph replay, problem 0 against
    the oracle at test_step_loads' tolerances, every workspace behind an untouched sentinel band."""
    x, y, xo, h, w, s = _dense_problem(B, d, n, M, 7000 * n + 10 * M + d + B)
    res = []
    for name, eng in engines:
        eng.set_guard(True)
        try:
            plan = eng.plan(B, d, n, M)
        finally:
            eng.set_guard(False)
        try:
            plan.set_inputs(x, y, xo, h, w, s)
            plan.run()
            r1 = plan.results()
            guarded, damaged = plan.check_guards()
            plan.run()  # (the graph replay)
            r2 = plan.results()
            guarded2, damaged2 = plan.check_guards()
        finally:
            plan.close()
        assert guarded >= 8 and damaged == 0 and damaged2 == 0, (name, guarded, damaged, damaged2)
        for a, b_ in zip(r1, r2):
            assert np.array_equal(a, b_), name
        res.append(r1)
    for (name, _), r in zip(engines[1:], res[1:]):
        for got, want in zip(r, res[0]):
            assert np.array_equal(got, want), name
    mean, var, logml, status = res[0]
    assert (status == 0).all()
    Lo, ao, lmo = oracle.gp_fit(x[0], y[0], h, w, s)
    mo, vo = oracle.gp_predict(x[0], h, w, Lo, ao, xo[0])
    assert np.max(np.abs(mean[0] - mo)) / np.max(np.abs(mo)) < 1e-10
    assert np.max(np.abs(var[0] - vo)) / oracle.kernel_scale(d, h, w) < 1e-10
    assert abs(logml[0] - lmo) <= 1e-10 * max(abs(lmo), 0.5 * n * np.log(2 * np.pi))


def test_readme_names_the_test_of_the_pipeline_switch():
    """README's list of switches has BQ_DIAG_PIPE with a test that exists in this file, and the
    one list of launch switches has it as a member that launch_slab_step reads."""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = " ".join(f.read().split())
    m = re.search(r"`BQ_DIAG_PIPE[^`]*`[^;]*?-- `test_diag_pipeline\.py::(test_\w+)`", text)
    assert m, "README has no BQ_DIAG_PIPE line that names a test of this file"
    assert callable(globals().get(m.group(1))), m.group(1)
    with open(os.path.join(ROOT, "bayesian-quadrature_amd", "csrc", "launch_config.h")) as f:
        assert re.search(r'X\(diag_pipe,\s*"BQ_DIAG_PIPE",\s*1\)', f.read())
    with open(os.path.join(ROOT, "bayesian-quadrature_amd", "csrc", "k_panel.hip")) as f:
        assert "cfg.diag_pipe" in f.read()
