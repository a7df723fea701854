"""The 16 x 16 block inverses of the diagonal factor's record (csrc/potf2.h, potf2f_block_inverse):
W_b = L_bb^-1 of the four diagonal sub-blocks of a factored 64 x 64 block, by a 4 x 4-blocked
recursion on v_mfma_f64_4x4x4_4b_f64, stored whole (column-major, the strict upper triangle exact
zeros) behind the 64 reciprocal pivots.  Every producer of a record -- the eight- and the four-wave
factor, the padded epilogue of a block of fewer than 64 columns, diag_winv_kernel for a resident
factor -- calls that one function on the same values, so two records of one factor are the same
BITS.  What can go wrong: an operand of a product taken from the wrong 4 x 4 block or transposed, a
block of W stored in another's place or not at all, a failing sub-block that reaches its neighbours.

The bar on an inverse is that of test_diag_pipeline.py: e_gpu <= 4 e_ref + 64 eps with
e = max |W_b L_bb - I| and e_ref the same residual of a float64 column-substitution inverse of the
same L_bb.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from conftest import rand_spd
from engine_env import engine_env
from test_cholesky_contracts import EPS
from test_slab_wave_groups import _bits, _matrix, _pack, _unpack
from test_step_loads import _dense_problem

gpu = pytest.mark.gpu

CONTEXTS = (("default", {}), ("four_waves", {"BQ_POTF2_8W": "0"}))


@pytest.fixture(scope="module")
def engines(engine):
    with contextlib.ExitStack() as stack:
        yield [(name, stack.enter_context(engine_env(env, probes=True))) for name, env in CONTEXTS]


def _probe_potf2(pe, A, flags, nreal=0):
    """bq_probe_potf2: (tril L, the record, info).  flags bit 0: the block handed over through LDS;
    bit 1: eight waves; nreal: the real columns of an identity-padded block (0: a full block)."""
    from bayesian_quadrature_amd import _lib as L
    A = np.asfortranarray(A, dtype=np.float64)
    Lo = np.zeros((64, 64), order="F")
    dv = np.zeros(64 + 4 * 256)
    info = C.c_int32(0)
    us = C.c_double(0)
    st = (C.c_int64 * 136)()
    pe._check(pe._lib.bq_probe_potf2(pe._ctx, L.dptr(A), flags | (nreal << 8), 2, L.dptr(Lo),
                                     L.dptr(dv), C.byref(info), C.cast(C.byref(us), L._dp), st))
    return np.tril(Lo), dv, info.value


def _w(dv, b):
    """W_b as stored: all 256 doubles, W[r][k] at r + 16 k."""
    return dv[64 + 256 * b:64 + 256 * (b + 1)].reshape(16, 16, order="F")


def _sub(Lo, b):
    return Lo[16 * b:16 * b + 16, 16 * b:16 * b + 16]


def _ref_inverse(Lb):
    """float64 forward substitution, unit column by unit column"""
    n = Lb.shape[0]
    W = np.zeros((n, n))
    for c in range(n):
        for i in range(c, n):
            W[i, c] = ((1.0 if i == c else 0.0) - Lb[i, c:i].dot(W[c:i, c])) / Lb[i, i]
    return W


def _resid(W, Lb):
    return float(np.max(np.abs(W.dot(Lb) - np.eye(Lb.shape[0]))))


def _check_inverses(Lo, dv, what, blocks=range(4)):
    for b in blocks:
        Lb, W = _sub(Lo, b), _w(dv, b)
        e_ref = _resid(_ref_inverse(Lb), Lb)
        assert np.isfinite(e_ref) and e_ref < 1e-8, (what, b, e_ref)
        assert np.all(np.triu(W, 1) == 0.0), (what, b)
        e_gpu = _resid(W, Lb)
        print("block inverse %s b %d e_gpu %.3e e_ref %.3e" % (what, b, e_gpu, e_ref))
        assert e_gpu <= 4 * e_ref + 64 * EPS, (what, b, e_gpu, e_ref)


def _blocks():
    """dense; graded (diagonal scales over six decades); sub-blocks of very different norms"""
    S = rand_spd(np.random.RandomState(41), 64)
    g = 10.0 ** np.linspace(3.0, -3.0, 64)
    rs = np.random.RandomState(43)
    g = g[rs.permutation(64)]
    nb = np.repeat([1.0, 3.0e4, 2.0e-5, 7.0e2], 16)
    return (("dense", S), ("graded", np.asfortranarray(S * np.outer(g, g))),
            ("block_norms", np.asfortranarray(S * np.outer(nb, nb))))


@gpu
@pytest.mark.parametrize("name,A", _blocks(), ids=[n for n, _ in _blocks()])
def test_inverse_of_every_sub_block(engine, name, A):
    """Every W_b inside the bar and upper-triangular zeros exact; four and eight waves, out of
    memory and through LDS: the same bits of factor and record."""
    pe = engine.probe_engine()
    outs = [_probe_potf2(pe, A, fl) for fl in (0, 1, 2, 3)]
    for fl, (Lo, dv, info) in enumerate(outs):
        assert info == 0, (name, fl)
        assert np.array_equal(_bits(Lo), _bits(outs[0][0])), (name, fl)
        assert np.array_equal(_bits(dv), _bits(outs[0][1])), (name, fl)
    _check_inverses(outs[0][0], outs[0][1], name)


@gpu
@pytest.mark.parametrize("nreal", [19, 63])
def test_padded_epilogue_agrees_with_the_full_one(engine, nreal):
    """An identity-padded block through the padded steps (their epilogue reads a copy of the
    sub-blocks) and as a full block (out of the panels' slots): where the two factors hold the same
    bits so do the inverses; every sub-block is inside the bar either way."""
    pe = engine.probe_engine()
    A = np.eye(64, order="F")
    A[:nreal, :nreal] = rand_spd(np.random.RandomState(47 + nreal), nreal)
    for fl in (0, 1, 2, 3):
        Lf, dvf, inff = _probe_potf2(pe, A, fl)
        Lp, dvp, infp = _probe_potf2(pe, A, fl, nreal)
        assert inff == 0 and infp == 0, (nreal, fl)
        _check_inverses(Lp, dvp, "padded %d flags %d" % (nreal, fl))
        shared = 0
        for b in range(4):
            if np.array_equal(_bits(_sub(Lp, b)), _bits(_sub(Lf, b))):
                shared += 1
                assert np.array_equal(_bits(_w(dvp, b)), _bits(_w(dvf, b))), (nreal, fl, b)
                assert np.array_equal(_bits(dvp[16 * b:16 * b + 16]),
                                      _bits(dvf[16 * b:16 * b + 16])), (nreal, fl, b)
        # (the real columns are factored by the same operations in both: at least the sub-blocks
        # that lie wholly in front of the padding are shared)
        assert shared >= nreal // 16, (nreal, fl, shared)


@gpu
def test_failing_pivot_in_sub_block_2_leaves_0_and_1_alone(engine):
    """Pivot 37 made non-positive: info is 38 in every form, and W_0, W_1 -- other waves' -- are the
    bits of the clean run."""
    pe = engine.probe_engine()
    S = rand_spd(np.random.RandomState(53), 64)
    Lr = np.linalg.cholesky(S)
    B = S.copy(order="F")
    B[37, 37] = Lr[37, :37].dot(Lr[37, :37]) - 1e-3
    for fl in (0, 1, 2, 3):
        _, dv0, info0 = _probe_potf2(pe, S, fl)
        _, dv, info = _probe_potf2(pe, B, fl)
        assert info0 == 0 and info == 38, (fl, info0, info)
        for b in (0, 1):
            assert np.array_equal(_bits(_w(dv, b)), _bits(_w(dv0, b))), (fl, b)
        assert np.array_equal(_bits(dv[:32]), _bits(dv0[:32])), fl


@gpu
@pytest.mark.parametrize("ntot", [128, 192, 320])
def test_sweep_same_bits_backward_error_and_replays(engines, ntot):
    """The one-launch steps on a dense matrix: the factor memory of the default context and of the
    four-wave factor are the same bits, the backward error is inside 1e-14 N, and ten replays give
    the first run's bits."""
    A = _matrix(ntot, 0)[0]
    src = _pack([A], ntot)
    outs = []
    for name, eng in engines:
        buf = src.copy()
        info, route = eng.probe_potrf_batch(buf, 1, ntot, None, ntot, ntot * ntot)
        assert route[0] == "slab" and not info.any(), (name, route, info)
        outs.append(buf)
    L0 = np.tril(_unpack(outs[0], 0, ntot, ntot))
    assert np.array_equal(_bits(L0), _bits(np.tril(_unpack(outs[1], 0, ntot, ntot)))), ntot
    berr = np.linalg.norm(L0.dot(L0.T) - A) / np.linalg.norm(A)
    print("block inverse sweep ntot %d backward error %.3e" % (ntot, berr))
    assert berr < 1e-14 * ntot, (ntot, berr)
    name, eng = engines[0]
    for rep in range(10):
        buf = src.copy()
        info, _ = eng.probe_potrf_batch(buf, 1, ntot, None, ntot, ntot * ntot)
        assert not info.any()
        assert np.array_equal(_bits(np.tril(_unpack(buf, 0, ntot, ntot))), _bits(L0)), (ntot, rep)


PLAN_CASES = [(1, d, n, M) for d in (1, 2) for n in (19, 63, 64, 65, 100) for M in (1, 10)]
PLAN_CASES.append((3, 2, 100, 10))


@gpu
@pytest.mark.parametrize("B,d,n,M", PLAN_CASES)
def test_plans_against_the_oracle_under_guards(engine, oracle, B, d, n, M):
    """Bordered plans whose leading block is padded (n < 64), full, or followed by a padded one:
every problem against the oracle at the project's 1e-10 bars, every workspace behind an untouched
    sentinel band, a replay the same bits."""
    x, y, xo, h, w, s = _dense_problem(B, d, n, M, 9000 * n + 10 * M + d + B)
    engine.set_guard(True)
    try:
        plan = engine.plan(B, d, n, M)
    finally:
        engine.set_guard(False)
    try:
        plan.set_inputs(x, y, xo, h, w, s)
        plan.run()
        r1 = plan.results()
        guarded, damaged = plan.check_guards()
        plan.run()
        r2 = plan.results()
        guarded2, damaged2 = plan.check_guards()
    finally:
        plan.close()
    assert guarded >= 1 and damaged == 0 and damaged2 == 0, (guarded, damaged, damaged2)
    for a, b_ in zip(r1, r2):
        assert np.array_equal(a, b_)
    mean, var, logml, status = r1
    assert (status == 0).all()
    for i in range(B):
        Lo, ao, lmo = oracle.gp_fit(x[i], y[i], h, w, s)
        mo, vo = oracle.gp_predict(x[i], h, w, Lo, ao, xo[i])
        assert np.max(np.abs(mean[i] - mo)) / np.max(np.abs(mo)) < 1e-10, i
        assert np.max(np.abs(var[i] - vo)) / oracle.kernel_scale(d, h, w) < 1e-10, i
        assert abs(logml[i] - lmo) <= 1e-10 * max(abs(lmo), 0.5 * n * np.log(2 * np.pi)), i


@gpu
def test_resident_record_is_the_sweeps_record(engine):
    """n = 128: the two records the one-launch steps leave behind (both halves of the ping-pong
    survive) against the records diag_winv_kernel builds from the factor in memory, as for a
    resident fit: reciprocal pivots and all four inverses of both blocks, the same bits."""
    A = _matrix(128, 0)[0]
    Lf, rec_sweep, rec_res, info = engine.probe_records(A)
    assert info == 0
    Lf = np.tril(Lf)
    for blk in range(2):
        assert np.array_equal(_bits(rec_sweep[blk]), _bits(rec_res[blk])), blk
        _check_inverses(Lf[64 * blk:64 * blk + 64, 64 * blk:64 * blk + 64], rec_res[blk],
                        "resident block %d" % blk)
