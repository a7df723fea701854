"""Workgroup 0's path through the one-launch Cholesky steps (csrc/potf2.h, csrc/slab.h): the
eight-wave diagonal factor (potf2f_run<8>), the hand-off of the updated diagonal block to it as
ten packed 16 x 16 blocks behind one barrier (slab_step_kernel<., 8>, slab_load_blocks8), the
assembly's own first factor, and every other kernel that instantiates the eight-wave factor.  The
four-wave forms (BQ_POTF2_8W=0, and the probe's flags 0 / 1) are the reference: the same
operations on the same operands in the same order, so the same BITS -- up to a failing pivot's
column as well.

The operands are DENSE (conftest.rand_spd, the 2-D problems of the batched tests): on the 1-D Gram
of the workloads most of a block's entries are exact zeros and a misplaced update cannot show.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from conftest import rand_spd
from test_cholesky_contracts import EPS, fwd_err
from engine_env import engine_env
from test_slab_wave_groups import _bits, _matrix, _pack, _unpack

gpu = pytest.mark.gpu

CONTEXTS = (("default", {}), ("four_waves", {"BQ_POTF2_8W": "0"}))


@pytest.fixture(scope="module")
def engines(engine):
    with contextlib.ExitStack() as stack:
        yield [(name, stack.enter_context(engine_env(env, probes=True))) for name, env in CONTEXTS]


# ---- the factor alone ---------------------------------------------------------------------------
def _probe_potf2(pe, A, flags):
    """bq_probe_potf2: (tril L, reciprocal pivots + block inverses, info).  flags bit 0: the block
    handed over through LDS; bit 1: eight waves."""
    from bayesian_quadrature_amd import _lib as L
    A = np.asfortranarray(A, dtype=np.float64)
    Lo = np.zeros((64, 64), order="F")
    dv = np.zeros(64 + 4 * 256)
    info = C.c_int32(0)
    us = C.c_double(0)
    st = (C.c_int64 * 136)()
    pe._check(pe._lib.bq_probe_potf2(pe._ctx, L.dptr(A), flags, 2, L.dptr(Lo), L.dptr(dv),
                                     C.byref(info), C.cast(C.byref(us), L._dp), st))
    return np.tril(Lo), dv, info.value


def _winv(dv, b):
    return np.tril(dv[64 + 256 * b:64 + 256 * (b + 1)].reshape(16, 16, order="F"))


# first and last column of a panel, the panel boundary, the second panel (another wave), the
# 16 x 16 sub-block boundary, the last panels
FAIL_COLS = (0, 3, 4, 7, 8, 15, 16, 56, 59, 60, 63)


@gpu
def test_factor_forms_agree_up_to_a_failing_pivot(engine):
    """A dense 64 x 64 block through the four forms of the probe (four / eight waves, from global
    memory / through LDS): without a failure L, the reciprocal pivots and the four block inverses
    are the same bits; with pivot c made non-positive every form reports c + 1 and the columns
    before c are the bits of the four-wave form from global memory."""
    pe = engine.probe_engine()
    S = rand_spd(np.random.RandomState(29), 64)
    Lr = np.linalg.cholesky(S)
    outs = [_probe_potf2(pe, S, fl) for fl in (0, 1, 2, 3)]
    assert np.max(np.abs(outs[0][0] - Lr)) <= 1e-13 * np.max(np.abs(Lr))
    for fl, (Lo, dv, info) in enumerate(outs):
        assert info == 0, fl
        assert np.array_equal(_bits(Lo), _bits(outs[0][0])), fl
        assert np.array_equal(_bits(dv[:64]), _bits(outs[0][1][:64])), fl
        for b in range(4):
            assert np.array_equal(_bits(_winv(dv, b)), _bits(_winv(outs[0][1], b))), (fl, b)
    for c in FAIL_COLS:
        B = S.copy(order="F")
        B[c, c] = Lr[c, :c].dot(Lr[c, :c]) - 1e-3
        ref = None
        for fl in (0, 1, 2, 3):
            Lo, dv, info = _probe_potf2(pe, B, fl)
            assert info == c + 1, (c, fl, info)
            if ref is None:
                ref = Lo
                assert np.array_equal(_bits(Lo[:, :c]), _bits(outs[0][0][:, :c])), c
            assert np.array_equal(_bits(Lo[:, :c]), _bits(ref[:, :c])), (c, fl)


# ---- through the sweep --------------------------------------------------------------------------
def _sweep(eng, src, batch, ntot, ld):
    buf = src.copy()
    info, route = eng.probe_potrf_batch(buf, batch, ntot, None, ld, ld * ntot)
    assert route[0] == "slab", route
    return buf, info


@gpu
@pytest.mark.parametrize("col", [64 + 3, 64 + 4, 64 + 7, 64 + 8, 127])
@pytest.mark.parametrize("batch,lda", [(1, 0), (3, 0), (3, 200)])
def test_sweep_reports_a_failing_pivot_of_workgroup_0(engines, batch, lda, col):
    """ntot = 192 on the one-launch steps: the block of columns 64 .. 127 is factored by workgroup 0
    of step 0.  A non-positive pivot planted there, in the last matrix of the batch: the same info
    from eight and four waves, the same bits in every column before it, and the clean matrices
    beside it whole."""
    ntot = 192
    ld = lda if lda else ntot
    mats = [_matrix(ntot, b)[0] for b in range(batch)]
    bad = mats[-1].copy(order="F")
    bad[col, col] = -5.0
    src = _pack(mats[:-1] + [bad], ld)
    want = np.zeros(batch, dtype=np.int32)
    want[-1] = col + 1
    outs = []
    for name, eng in engines:
        buf, info = _sweep(eng, src, batch, ntot, ld)
        assert np.array_equal(info, want), (name, info)
        outs.append(buf)
    for b in range(batch - 1):
        assert np.array_equal(_bits(_unpack(outs[0], b, ntot, ld)),
                              _bits(_unpack(outs[1], b, ntot, ld))), b
    got8 = np.tril(_unpack(outs[0], batch - 1, ntot, ld))[:, :col]
    got4 = np.tril(_unpack(outs[1], batch - 1, ntot, ld))[:, :col]
    assert np.array_equal(_bits(got8), _bits(got4))
    # (the columns of the blocks in front of the failing one are final and finite)
    assert np.isfinite(got8[:, :64]).all()


@gpu
@pytest.mark.parametrize("ntot", [128, 192])
def test_hand_off_of_the_diagonal_block(engines, ntot):
    """ntot = 128: one step, one workgroup -- only the hand-off of the updated diagonal block to
    the factor; ntot = 192: a second step and two more tiles.  Eight waves against four: the same
    bits; and within 4 e_ref + 64 eps of the long-double column Cholesky (e_ref: LAPACK's own
    forward error on the matrix)."""
    A, L, e_ref = _matrix(ntot, 0)
    src = _pack([A], ntot)
    outs = []
    for name, eng in engines:
        buf, info = _sweep(eng, src, 1, ntot, ntot)
        assert not info.any(), (name, info)
        outs.append(buf)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    e_gpu = fwd_err(np.tril(_unpack(outs[0], 0, ntot, ntot)), L)
    print("corner hand-off ntot %d e_gpu %.3e e_ref %.3e" % (ntot, e_gpu, e_ref))
    assert e_gpu <= 4 * e_ref + 64 * EPS, (ntot, e_gpu, e_ref)


# ---- the first launch ---------------------------------------------------------------------------
def _problem(B, d, n, M, seed):
    """(x, y, xo, h, w, s) of B problems: d = 1 as test_gpu_parity's folded read-out builds them,
    d = 2 dense as its batched tests do."""
    from bayesian_quadrature_amd import workloads as wl
    rs = np.random.RandomState(seed)
    if d == 1:
        dx = 10.0 / n
        x = np.linspace(-5, 5, n)[None, :] + 0.2 * dx * rs.uniform(-1, 1, (B, n))
        y = np.sin(x) + 0.1 * rs.randn(B, n)
        return x, y, rs.uniform(-5, 5, (B, M)), 1.3, np.array([1.3 * dx]), 1e-3
    x = rs.uniform(-3, 3, (B, d, n))
    y = wl.norm_logpdf(x[:, 0]) + wl.norm_logpdf(x[:, 1])
    return x, y, rs.uniform(-3, 3, (B, d, M)), 1.3, np.full(d, 6.0 / np.sqrt(n) * 1.5), 0.05


FIRST_CASES = [(1, d, n, M) for d in (1, 2) for n in (19, 63, 64, 65, 100) for M in (1, 10)]
FIRST_CASES.append((3, 2, 65, 10))


@gpu
@pytest.mark.parametrize("B,d,n,M", FIRST_CASES)
def test_first_launch_leading_block(engines, oracle, B, d, n, M):
    """The assembly's own factor of the leading block (assemble_first_kernel): a padded block
    (n < 64) and a full one, a border that reaches into tile (0, 0) and one that does not.  mean /
    var / logml / status: eight waves against four the same bits, problem 0 against the oracle at
    the tolerances of test_gpu_parity's plans."""
    x, y, xo, h, w, s = _problem(B, d, n, M, 100 * n + 10 * M + d)
    res = []
    for name, eng in engines:
        plan = eng.plan(B, d, n, M)
        plan.set_inputs(x, y, xo, h, w, s)
        plan.run()
        res.append(plan.results())
        plan.close()
    for got, want in zip(res[0], res[1]):
        assert np.array_equal(got, want)
    mean, var, logml, status = res[0]
    assert (status == 0).all()
    Lo, ao, lmo = oracle.gp_fit(x[0], y[0], h, w, s)
    mo, vo = oracle.gp_predict(x[0], h, w, Lo, ao, xo[0])
    assert np.max(np.abs(mean[0] - mo)) / np.max(np.abs(mo)) < 1e-10
    assert np.max(np.abs(var[0] - vo)) / oracle.kernel_scale(d, h, w) < 1e-10
    assert abs(logml[0] - lmo) <= 1e-10 * max(abs(lmo), 0.5 * n * np.log(2 * np.pi))


# ---- the other kernels that instantiate the eight-wave factor -----------------------------------
def _launches(eng, fn):
    """fn() under the launch profiler: launches per class."""
    eng.profile(True)
    eng.profile_reset()
    try:
        out = fn()
        eng.sync()
        return out, {k: v["launches"] for k, v in eng.profile_read().items()}
    finally:
        eng.profile(False)


def _potrf_dev(eng, A):
    n = A.shape[0]
    dA, dinfo = eng.alloc(8 * n * n), eng.alloc(64)
    try:
        eng.upload(dA, A)
        st = eng._lib.bq_potrf_dev(eng._ctx, dA, n, n, dinfo)
        hinfo = np.full(1, -7, dtype=np.int32)
        eng.download(hinfo, dinfo)
        out = np.empty(n * n)
        eng.download(out, dA)
        return st, int(hinfo[0]), out
    finally:
        eng.free(dA), eng.free(dinfo)


@gpu
def test_lone_factor_launch_eight_waves(engines):
    """potf2_kernel<8> (trsm.h): a 64 x 64 system is one launch of the diagonal factor."""
    A = _matrix(64, 0)[0]
    outs = []
    for name, eng in engines:
        (buf, info), cnt = _launches(eng, lambda: _sweep(eng, _pack([A], 64), 1, 64, 64))
        assert not info.any() and cnt["potf2"] == 1, (name, info, cnt)
        assert sum(cnt.values()) == 1, (name, cnt)
        outs.append(buf)
    assert np.array_equal(_bits(np.tril(_unpack(outs[0], 0, 64, 64))),
                          _bits(np.tril(_unpack(outs[1], 0, 64, 64))))


@gpu
def test_panel_step_smallest_eight_waves(engines):
    """panel_step_kernel<8>: bq_potrf_dev on a dense n = 128 matrix under set_block(128) is the
    lone factor of the first block and ONE step of the wide panel, whose workgroup 0 factors the
    second block -- no panel solve of its own, no trailing update."""
    n = 128
    A, L, e_ref = _matrix(n, 0)
    outs = []
    for name, eng in engines:
        try:
            eng.set_block(128)
            (st, info, out), cnt = _launches(eng, lambda: _potrf_dev(eng, A))
        finally:
            eng.set_block(0)
        assert (st, info) == (0, 0), (name, st, info)
        assert cnt["potf2"] == 1 and cnt["gemm_panel"] == 1 and cnt["trsm"] == 0, (name, cnt)
        outs.append(np.tril(out.reshape(n, n).T))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert fwd_err(outs[0], L) <= 4 * e_ref + 64 * EPS


@gpu
def test_workgroup_per_matrix_eight_waves(engine):
    """potrf_wg_kernel (a batch's diagonal blocks, one workgroup per matrix; BQ_DF_WG=1 makes it
    the diagonal factor at any batch size): 70 x 512 is the smallest batch the rule gives an outer
    block of 128 -- the diag_first route.  The kernel has no four-wave form, so besides the bits
    of a BQ_POTF2_8W=0 context the leading 64 x 64 block of every sampled factor is compared with
    the four-wave probe's factor of the same block."""
    batch, ntot = 70, 512
    mats = [_matrix(ntot, b % 2)[0] for b in range(batch)]
    src = _pack(mats, ntot)
    outs = []
    for env in ({"BQ_DF_WG": "1"}, {"BQ_DF_WG": "1", "BQ_POTF2_8W": "0"}):
        with engine_env(env, probes=True) as eng:
            buf = src.copy()
            info, route = eng.probe_potrf_batch(buf, batch, ntot, None, ntot, ntot * ntot)
            assert route[0] == "diag_first" and route[1] == 128 and not info.any(), (route, info)
            outs.append(buf)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    pe = engine.probe_engine()
    for b in (0, 1, batch - 1):
        Lo, dv, info = _probe_potf2(pe, mats[b][:64, :64], 0)
        got = np.tril(_unpack(outs[0], b, ntot, ntot)[:64, :64])
        assert info == 0 and np.array_equal(_bits(got), _bits(Lo)), b
