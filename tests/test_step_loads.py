"""The prologue of the one-launch Cholesky steps (csrc/slab.h, slab_step_kernel): every global
load of a step -- fragments, panel rows, the C tile -- is issued in one straight run, the tile RAW
(it is negated in front of the update), and a diagonal tile's blocks are loaded without a branch:
waves 2 and 3 load their second 16 x 16 block again as a third, and every wave its third as a
fourth, into accumulators that nothing stores.  What can go wrong is a block loaded from the wrong
place, a duplicate stored where a wave's own block was meant, or a sign lost -- so everything here
is checked on the values, eight waves against four (BQ_POTF2_8W=0: the same operations on the same
operands in the same order, the same BITS) and against references on the host.

The operands are DENSE (conftest.rand_spd; random points under a wide kernel): on the 1-D Gram of
the workloads most of a tile is exact zeros, and a block loaded from the wrong place cannot show.
"""
import contextlib

import numpy as np
import pytest

from test_cholesky_contracts import EPS, fwd_err, ld_cholesky
from engine_env import engine_env
from test_slab_wave_groups import _bits, _matrix, _pack, _unpack

gpu = pytest.mark.gpu

CONTEXTS = (("default", {}), ("four_waves", {"BQ_POTF2_8W": "0"}))


@pytest.fixture(scope="module")
def engines(engine):
    with contextlib.ExitStack() as stack:
        yield [(name, stack.enter_context(engine_env(env, probes=True))) for name, env in CONTEXTS]


def _factor_both(engines, src, batch, ntot, ld):
    """probe_potrf_batch of `src` in both contexts: the two buffers (same bits, asserted) and
    info."""
    outs, infos = [], []
    for name, eng in engines:
        buf = src.copy()
        info, route = eng.probe_potrf_batch(buf, batch, ntot, None, ld, ld * ntot)
        assert route[0] == "slab", (name, route)
        outs.append(buf)
        infos.append(info)
    assert np.array_equal(infos[0], infos[1]), infos
    for b in range(batch):
        lo8 = np.tril(_unpack(outs[0], b, ntot, ld))
        lo4 = np.tril(_unpack(outs[1], b, ntot, ld))
        assert np.array_equal(_bits(lo8), _bits(lo4)), (ntot, b)
    return outs[0], infos[0]


def _check_against_numpy(A, L_ld, L_gpu, what):
    """The bound of test_cholesky_contracts: e_gpu <= 4 e_ref + 64 eps against the long-double
    column Cholesky, e_ref = the forward error of the fp64 reference -- here numpy.linalg.cholesky
    -- on the same matrix.  Hence, by the triangle inequality, 5 e_ref + 64 eps against numpy's
    factor itself."""
    Lnp = np.linalg.cholesky(A)
    e_ref, e_gpu = fwd_err(Lnp, L_ld), fwd_err(L_gpu, L_ld)
    e_np = fwd_err(L_gpu, Lnp.astype(np.longdouble))
    print("step loads %s e_gpu %.3e e_ref %.3e vs numpy %.3e" % (what, e_gpu, e_ref, e_np))
    assert e_gpu <= 4 * e_ref + 64 * EPS, (what, e_gpu, e_ref)
    assert e_np <= 5 * e_ref + 64 * EPS, (what, e_np, e_ref)


# ntot = 128: one step, a lone diagonal tile; 192: the first off-diagonal tile; 256, 320: tile
# column 0 goes to the scratch column, two and three ping-pong steps
@gpu
@pytest.mark.parametrize("batch,pad", [(1, 0), (3, 0), (3, 8)])
@pytest.mark.parametrize("ntot", [128, 192, 256, 320])
def test_sweep_same_bits_and_within_the_contract_bound(engines, ntot, batch, pad):
    ld = ntot + pad
    mats = [_matrix(ntot, b) for b in range(batch)]
    out, info = _factor_both(engines, _pack([m[0] for m in mats], ld), batch, ntot, ld)
    assert not info.any(), info
    for b, (A, L, _) in enumerate(mats):
        _check_against_numpy(A, L, np.tril(_unpack(out, b, ntot, ld)),
                             "ntot %d batch %d ld %d b %d" % (ntot, batch, ld, b))


# the ten lower 16 x 16 blocks of a diagonal tile as slab_diag_rb / slab_diag_cb deal them to the waves
BLOCKS = [(rb, cb) for rb in range(4) for cb in range(rb + 1)]
_BASE = {}


def _base192(engines):
    if not _BASE:
        A, L, _ = _matrix(192, 0)
        out, info = _factor_both(engines, _pack([A], 192), 1, 192, 192)
        assert not info.any()
        _BASE["L"] = np.tril(_unpack(out, 0, 192, 192)).copy()
    return _BASE["L"]


# t0 = 64: the tile that workgroup 0 updates and hands to the factor through LDS (the packed
# blocks); t0 = 128: the diagonal tile that goes back to memory (the stores under slab_diag_nb)
@gpu
@pytest.mark.parametrize("t0", [64, 128])
@pytest.mark.parametrize("rb,cb", BLOCKS)
def test_every_diagonal_block_is_its_own(engines, rb, cb, t0):
    """One entry inside block (rb, cb) of the diagonal tile at t0 moved: the factor moves there
    (a wave that loaded its duplicate where this block was meant would not see it), eight and
    four waves agree bit for bit, and the result is the moved matrix's factor."""
    A0, _, _ = _matrix(192, 0)
    base = _base192(engines)
    A = A0.copy(order="F")
    i, k = t0 + 16 * rb + 9, t0 + 16 * cb + 5   # below the diagonal in a diagonal block too
    A[i, k] += 0.375
    A[k, i] = A[i, k]
    out, info = _factor_both(engines, _pack([A], 192), 1, 192, 192)
    assert not info.any()
    Lg = np.tril(_unpack(out, 0, 192, 192))
    assert Lg[i, k] != base[i, k], (rb, cb, t0)
    L_ld, linfo = ld_cholesky(A)
    assert linfo == 0
    _check_against_numpy(A, L_ld, Lg, "block (%d, %d) of the tile at %d" % (rb, cb, t0))


def _dense_problem(B, d, n, M, seed):
    """B problems on random points under a wide kernel (as test_gpu_parity's dense batches, in one
    dimension too): no tile of the bordered system is zeros."""
    from bayesian_quadrature_amd import workloads as wl
    rs = np.random.RandomState(seed)
    x = rs.uniform(-3, 3, (B, d, n))
    xo = rs.uniform(-3, 3, (B, d, M))
    y = sum(wl.norm_logpdf(x[:, j]) for j in range(d))
    if d == 1:
        x, xo = x[:, 0], xo[:, 0]
    return x, y, xo, 1.3, np.full(d, 6.0 / np.sqrt(n) * 1.5), 0.05


PLAN_CASES = [(1, d, n, M) for d in (1, 2) for n in (65, 128, 200) for M in (1, 70)]
PLAN_CASES.append((3, 2, 200, 70))


@gpu
@pytest.mark.parametrize("B,d,n,M", PLAN_CASES)
def test_plan_read_out_same_bits_oracle_and_guards(engines, oracle, B, d, n, M):
    """The bordered plan: the last step emits mean / var / log-ML from its tiles.  Eight waves
    against four the same bits; problem 0 against the oracle at test_gpu_parity's tolerances for
    its dense plans; every workspace behind a sentinel band that both passes leave alone."""
    x, y, xo, h, w, s = _dense_problem(B, d, n, M, 1000 * n + 10 * M + d)
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
    for got, want in zip(res[0], res[1]):
        assert np.array_equal(got, want)
    mean, var, logml, status = res[0]
    assert (status == 0).all()
    Lo, ao, lmo = oracle.gp_fit(x[0], y[0], h, w, s)
    mo, vo = oracle.gp_predict(x[0], h, w, Lo, ao, xo[0])
    assert np.max(np.abs(mean[0] - mo)) / np.max(np.abs(mo)) < 1e-10
    assert np.max(np.abs(var[0] - vo)) / oracle.kernel_scale(d, h, w) < 1e-10
    # (test_gpu_parity, test_batch_rule_boundaries: relative to the size of the log-ML's own terms)
    assert abs(logml[0] - lmo) <= 1e-10 * max(abs(lmo), 0.5 * n * np.log(2 * np.pi))
