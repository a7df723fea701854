"""The one-launch steps' wave groups (csrc/slab.h): in the 512-thread forms waves 4-7 solve one
row block while waves 0-3 solve the other (slab_step_kernel<., 8> off-diagonal tiles,
panel_step_kernel<8>), and launch_slab_step launches that form by a rule in rounds of workgroups
per CU (BQ_SLAB8_ROUNDS).  Same operations on the same operands in the same order as the
four-wave forms: every context below must give the same BITS.

The operands are DENSE: on the 1-D Gram of the workloads the far tiles are exact zeros and a
wrong solve of the Q rows cannot show.
"""
import contextlib
import os
import re

import numpy as np
import pytest

from conftest import rand_spd
from engine_env import engine_env
from test_cholesky_contracts import EPS, fwd_err, ld_cholesky

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# default; the 512-thread slab step at every size; one workgroup per CU (the rule before the
# rounds); four waves everywhere
CONTEXTS = (("default", {}), ("always", {"BQ_SLAB8_ROUNDS": "1000000"}),
            ("one_round", {"BQ_SLAB8_ROUNDS": "0"}), ("four_waves", {"BQ_POTF2_8W": "0"}))


@pytest.fixture(scope="module")
def engines(engine):
    with contextlib.ExitStack() as stack:
        yield [(name, stack.enter_context(engine_env(env, probes=True))) for name, env in CONTEXTS]


_REF = {}


def _matrix(n, idx):
    """(A, long-double factor, e_ref) of the dense SPD matrix `idx` of size n, cached: A + A^T +
    n I (conftest.rand_spd); e_ref = the forward error of LAPACK's dpotrf."""
    if (n, idx) not in _REF:
        from scipy.linalg import lapack
        A = rand_spd(np.random.RandomState(4099 * n + idx), n)
        L, info = ld_cholesky(A)
        assert info == 0
        L64, i64 = lapack.dpotrf(A, lower=1)
        assert i64 == 0
        _REF[(n, idx)] = (A, L, fwd_err(np.tril(L64), L))
    return _REF[(n, idx)]


def _pack(mats, lda):
    """The matrices column-major with leading dimension lda in one flat buffer, padding = NaN."""
    n = mats[0].shape[0]
    buf = np.full(lda * n * len(mats), np.nan)
    for b, A in enumerate(mats):
        buf[b * lda * n:(b + 1) * lda * n].reshape(n, lda)[:, :n] = A.T
    return buf


def _unpack(buf, b, n, lda):
    return buf[b * lda * n:(b + 1) * lda * n].reshape(n, lda)[:, :n].T


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# (ntot = 256, 384: steps of 3 .. 5 tiles per side -- the corner, the other tiles of column 0,
# interior off-diagonal tiles, diagonal tiles)
CASES = [(256, 1, 0), (384, 1, 0), (256, 3, 0), (384, 3, 392)]


@gpu
@pytest.mark.parametrize("ntot,batch,lda", CASES)
def test_dense_factor_same_bits_in_every_context(engines, ntot, batch, lda):
    """probe_potrf_batch on dense matrices: the factor is the same bits from every context and
    within 4 e_ref + 64 eps of the long-double column Cholesky."""
    ld = lda if lda else ntot
    mats = [_matrix(ntot, b) for b in range(batch)]
    src = _pack([m[0] for m in mats], ld)
    out = []
    for name, eng in engines:
        buf = src.copy()
        info, route = eng.probe_potrf_batch(buf, batch, ntot, None, ld, ld * ntot)
        assert route[0] == "slab" and not info.any(), (name, route, info)
        out.append(buf)
    for (name, _), buf in zip(engines[1:], out[1:]):
        assert np.array_equal(_bits(buf), _bits(out[0])), name
    for b, (A, L, e_ref) in enumerate(mats):
        e_gpu = fwd_err(np.tril(_unpack(out[0], b, ntot, ld)), L)
        print("slab8 ntot %d batch %d b %d e_gpu %.3e e_ref %.3e" % (ntot, batch, b, e_gpu, e_ref))
        assert e_gpu <= 4 * e_ref + 64 * EPS, (ntot, b, e_gpu, e_ref)


@gpu
@pytest.mark.parametrize("col", [70, 200])
@pytest.mark.parametrize("ntot,batch,lda", CASES)
def test_planted_pivot_same_info_in_every_context(engines, ntot, batch, lda, col):
    """One non-positive pivot planted in the last matrix of the batch: every context reports its
    column (1-based), and a clean matrix beside it reports none."""
    ld = lda if lda else ntot
    mats = [_matrix(ntot, b)[0] for b in range(batch)]
    bad = mats[-1].copy(order="F")
    bad[col, col] = -5.0
    src = _pack(mats[:-1] + [bad], ld)
    want = np.zeros(batch, dtype=np.int32)
    want[-1] = col + 1
    for name, eng in engines:
        info, route = eng.probe_potrf_batch(src.copy(), batch, ntot, None, ld, ld * ntot)
        assert route[0] == "slab" and np.array_equal(info, want), (name, route, info)


@gpu
@pytest.mark.parametrize("B", [1, 3])
def test_bordered_plan_same_bits_in_every_context(engines, oracle, B):
    """plan(B, 1, 200, 70): 384 rows with the border.  mean / var / logml / status are the same
    bits from every context; problem 0 is within 1e-10 of the oracle."""
    n, M = 200, 70
    rs = np.random.RandomState(23 + B)
    dx = 10.0 / n
    x = np.linspace(-5, 5, n)[None, :] + 0.2 * dx * rs.uniform(-1, 1, (B, n))
    y = np.sin(x) + 0.1 * rs.randn(B, n)
    xo = rs.uniform(-5, 5, (B, M))
    h, wv, s = 1.3, np.array([1.3 * dx]), 1e-3
    res = []
    for name, eng in engines:
        plan = eng.plan(B, 1, n, M)
        plan.set_inputs(x, y, xo, h, wv, s)
        plan.run()
        res.append(plan.results())
        plan.close()
    for (name, _), r in zip(engines[1:], res[1:]):
        for got, want in zip(r, res[0]):
            assert np.array_equal(got, want), name
    mean, var, logml, status = res[0]
    assert (status == 0).all()
    Lo, ao, lmo = oracle.gp_fit(x[0], y[0], h, wv, s)
    mo, vo = oracle.gp_predict(x[0], h, wv, Lo, ao, xo[0])
    k0 = oracle.kernel_scale(1, h, wv)
    assert np.max(np.abs(mean[0] - mo)) / np.max(np.abs(mo)) < 1e-10
    assert np.max(np.abs(var[0] - vo)) / k0 < 1e-10
    assert abs(logml[0] - lmo) / abs(lmo) < 1e-10


def _potrf_dev(eng, A):
    """bq_potrf_dev on the n x n matrix A (lda = n): (status, info, the buffer afterwards)."""
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
@pytest.mark.parametrize("lookahead", [True, False])
def test_panel_step_eight_waves_same_bits(engines, lookahead):
    """panel_step_kernel: bq_potrf_dev on a dense n = 640 matrix under set_block(256) -- the first
    step of a panel out of A, the side buffer, steps with and without a next slab, the last
    slab.  Eight waves against BQ_POTF2_8W=0: the same bits, and the same info for a pivot
    planted in the second slab."""
    n = 640
    A, L, e_ref = _matrix(n, 0)
    bad = A.copy(order="F")
    bad[100, 100] = -5.0
    got = []
    for name, eng in engines:
        if name not in ("default", "four_waves"):
            continue
        try:
            eng.set_block(256)
            eng.set_lookahead(lookahead)
            st, info, out = _potrf_dev(eng, A)
            assert (st, info) == (0, 0), (name, st, info)
            st, info, _ = _potrf_dev(eng, bad)
            assert (st, info) == (0, 101), (name, st, info)
            got.append(out)
        finally:
            eng.set_block(0)
            eng.set_lookahead(True)
    assert np.array_equal(_bits(got[0]), _bits(got[1]))
    e_gpu = fwd_err(np.tril(got[0].reshape(n, n).T), L)
    assert e_gpu <= 4 * e_ref + 64 * EPS, (e_gpu, e_ref)


def test_readme_names_the_test_of_the_rounds_switch():
    """README's list of switches has BQ_SLAB8_ROUNDS with a test that exists in this file."""
    with open(os.path.join(ROOT, "README.md")) as f:
        text = " ".join(f.read().split())
    m = re.search(r"`BQ_SLAB8_ROUNDS[^`]*`[^;]*?-- `(test_\w+)`", text)
    assert m, "README has no BQ_SLAB8_ROUNDS line that names a test"
    assert callable(globals().get(m.group(1))), m.group(1)
    with open(os.path.join(ROOT, "bayesian-quadrature_amd", "csrc", "launch_config.h")) as f:
        assert '"BQ_SLAB8_ROUNDS"' in f.read()
