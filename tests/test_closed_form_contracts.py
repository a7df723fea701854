"""The closed-form layer on the device, per entry and in every dimension: the Gram kernels of
csrc/gram.h (bq_gram_gauss, bq_gram_gauss_dev, bq_gram_gauss_cross), the four Gaussian integrals of
csrc/moments.h / moments.hip and E[Z], V(Z) on resident fits, each D = 1 .. 8 that BQ_DISPATCH_D
instantiates, against the long-double references of ld_closed_forms.py -- joint Gaussian densities
through one Cholesky factor, which share no algebra with the device.  References, units, bars and
their derivations are in that module's docstring; test_closed_form_contracts_host.py checks them
on the CPU and records r per case.

Gram.  Sizes cross the kernels' seams: n % 64 == 0 takes gram_tri_kernel (192: a three-block
triangle, tri_decode beyond 2 x 2), 63 / 65 / 129 gram_sym_kernel's odd and even tails.  Points:
a cluster and outliers under length scales 30 apart, so that exponents run from 0 to below -745.
Per entry the error is at most 2 ((D + 5) |q_ij| + 3 D + 4) ulps of the long-double value rounded
to float64, the spacing floored at the subnormal one: gauss_q costs 6 roundings per term
(subtract, square, times nh, and nh's own 2) plus D - 1 sums, all of one sign; make_params' c
costs 3 D + 1; the exp 1 ulp (test_exp_gauss_accuracy_on_probe_library); the product 1; the
reference's rounding 1; the factor 2 converts relative error to ulps.  K == K.T exactly; the
diagonal is within 4 ulps of c + s^2, c as make_params rounds it; rows [n, ldk) keep their bits;
an odd ldk (no 16-byte stores) gives the bits of the even one.

Integrals.  |got - ref| / |ref| <= MARGIN max(r, 4 eps) (1 + |E_ij|), E_ij the reference's log of
the entry over the largest, r measured from the cancellation-free float64 forms.  Families: the
existing tests' parameters (mild); the correlated, off-centre measure of test_gp_zdesign (corr) and
the same at rho = 0.9 (rho9); length scales 30 apart (aniso); measures wide against the length
scales, cov / w^2 = 4e4 -- the benchmark's C2 -- and 4e6, d = 1 .. 3 (wide4e4, wide4e6).

Measured (MI355X), the largest error in units of the bar over all sizes, d = 1 .. 3 left to right.
Before the fix of csrc/moments.hip (Cm = W2 + 2 S - 2 S (W1 + S)^-1 S and a Cholesky sweep over all
of [[S + W1, S], [S, S + W2]]): int_K1_K2 9.9 5.4 28.8 (wide4e4) and 18.5 19.6 29.2 (wide4e6),
int_int_K1_K2_K1 34.3 30.9 25.9 and 16.3 26.3 31.2, V(Z) of the wide d = 2 case 1.02.  After it
(cond_cov: W1 - W1 (W1 + S)^-1 W1, the factor of C2 by blocks): 0.015 0.009 0.019 and 0.009 0.013
0.014, 0.009 0.008 0.010 and 0.010 0.010 0.010, V(Z) 0.020.  Every other family and entry point,
d = 1 .. 8, before and after: at most 0.05, but for aniso d = 1 before the fix (0.09 and 0.22).
Gram: at most 0.27 of the bound at every d.  docs/LABBOOK.md, "The closed-form layer per entry",
has the table per entry point and d.

Moments.  E[Z] within MARGIN max(r_mean, 4 eps) sum |alpha_i kappa_i|; V(Z) = t1 - t2 within
MARGIN max(r_Z, 4 eps) |t1|, r_mean and r_Z the errors of the float64 restatement (numpy's Cholesky
solves around the cancellation-free integrals) against long double.  t2 / t1 is 0.52 .. 0.71 at
d = 8, 0.917 .. 0.9993 at d = 2, 0.989 .. 0.9998 at d = 3 and 0.999992 .. 0.999997 at d = 1: V(Z)
keeps five to six digits fewer than its terms there."""
import numpy as np
import pytest

import ld_closed_forms as F
from test_cholesky_contracts import SENTINEL

pytestmark = pytest.mark.gpu

FAM_D = [(fam, d) for fam in F.FAMILIES for d in F.family_dims(fam)]


def _gram_dev(engine, c, ldk):
    """bq_gram_gauss_dev into a buffer of leading dimension ldk filled with the payload NaN; the
    rows [n, ldk) of every column must come back as they were."""
    from bayesian_quadrature_amd import _lib as L_
    d, n = c["x"].shape
    xd, Kd = engine.alloc(8 * n * d), engine.alloc(8 * ldk * n)
    try:
        engine.upload(xd, c["x"])
        host = np.empty(ldk * n)
        host.view(np.uint64)[:] = SENTINEL
        engine.upload(Kd, host)
        engine._check(engine._lib.bq_gram_gauss_dev(engine._ctx, xd, d, n, c["h"], L_.dptr(c["w"]),
                                                    c["s"], Kd, ldk))
        engine.download(host, Kd)
    finally:
        engine.free(Kd)
        engine.free(xd)
    R = host.reshape(n, ldk)
    assert (R[:, n:].view(np.uint64) == SENTINEL).all(), ("rows [n, ldk) written", n, ldk)
    return np.asfortranarray(R[:, :n].T)


@pytest.mark.parametrize("n", F.GRAM_SIZES)
@pytest.mark.parametrize("d", F.D_ALL)
def test_gram_per_entry(engine, d, n):
    """bq_gram_gauss and bq_gram_gauss_dev (ldk = n + 2 > n): the per-entry bar, exact symmetry,
    the diagonal, and the same bits from both entry points."""
    c = F.gram_case(d, n)
    K = engine.gram(c["x"], c["h"], c["w"], c["s"])
    worst = F.check_gram(K, c)
    Kd = _gram_dev(engine, c, n + 2)
    F.check_gram(Kd, c)
    assert np.array_equal(K.view(np.uint64), Kd.view(np.uint64))
    print("units gram d=%d n=%d %.3f" % (d, n, worst))


@pytest.mark.parametrize("n", [64, 128, 192])
@pytest.mark.parametrize("d", F.D_ALL)
def test_gram_odd_ldk_same_bits(engine, d, n):
    """An odd ldk cannot take 16-byte stores: the call must fall to the scalar stores of
    gram_sym_kernel, give the bits of the even-ldk call (gram_tri_kernel) and leave rows
    [n, ldk) alone."""
    c = F.gram_case(d, n)
    even, odd = _gram_dev(engine, c, n + 2), _gram_dev(engine, c, n + 1)
    assert np.array_equal(even.view(np.uint64), odd.view(np.uint64))
    F.check_gram(odd, c)


@pytest.mark.parametrize("n1,n2", F.CROSS_SIZES)
@pytest.mark.parametrize("d", F.D_ALL)
def test_gram_cross_per_entry(engine, d, n1, n2):
    c = F.cross_case(d, n1, n2)
    worst = F.check_gram(engine.gram_cross(c["x1"], c["x2"], c["h"], c["w"]), c, cross=True)
    print("units gram_cross d=%d %dx%d %.3f" % (d, n1, n2, worst))


@pytest.mark.parametrize("name", ["int_K", "int_K1_K2", "int_int_K1_K2", "int_int_K1_K2_K1"])
@pytest.mark.parametrize("fam,d", FAM_D)
def test_integral_per_entry(engine, fam, d, name):
    """Every size of the entry point; int_int_K1_K2_K1 must also be symmetric to the bit (the
    kernel's arithmetic is symmetric term by term).  Every size runs before the first assertion
    speaks, so that the recorded figure is the family's largest."""
    worst, failed = 0.0, []
    for size in F.integral_sizes(name, d):
        c = F.integral_case(fam, d, name, size)
        assert F.all_normal(c[name])
        got = getattr(engine, name)(*c["args"])
        try:
            worst = max(worst, F.check_integral(got, c, name, symmetric=name.endswith("K1")))
        except AssertionError as e:
            failed.append((size, e.args[0]))
            if isinstance(e.args[0], tuple) and len(e.args[0]) > 1:
                worst = max(worst, e.args[0][1])
    print("units %s %s d=%d %.3f" % (name, fam, d, worst))
    assert not failed, (fam, d, name, failed)


@pytest.mark.parametrize("case", F.MOMENT_CASES, ids=lambda c: "d%d-%d-%d-s%g-%s" % c)
def test_moments(engine, case):
    """bq_bq_Z_mean and bq_bq_Z_var on resident fits: the fused alpha / beta reductions of
    int_K_kernel, int_int_K1_K2_K1_kernel and int_K1_K2_kernel and the forward sweep; nsc = 270
    crosses the fused reduction's 256-column strip and 64-row blocks."""
    c = F.moment_case(*case)
    assert float(c["zv"]) >= 0.0
    (h1, w1, s1), (h2, w2, s2) = c["p_tl"], c["p_l"]
    f1 = engine.gp_fit(c["xs"], np.log(c["ls"]), h1, w1, s1)
    f2 = engine.gp_fit(c["xsc"], c["lsc"], h2, w2, s2)
    try:
        zm, zv = engine.Z_mean(f2, c["mu"], c["cov"]), engine.Z_var(f1, f2, c["mu"], c["cov"])
    finally:
        f1.close(), f2.close()
    um = float(abs(F.LD(zm) - c["zm"]) / c["zabs"]) / F.integral_bar(c["r_mean"])
    uv = float(abs(F.LD(zv) - c["zv"]) / abs(c["t1"])) / F.integral_bar(c["r_Z"])
    print("units moments %s Z_mean %.3f Z_var %.3f t2/t1 %.6f" % (case, um, uv, c["ratio"]))
    F.check_Z_mean(zm, c)
    F.check_Z_var(zv, c)
