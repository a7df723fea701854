"""CPU tests of what test_closed_form_contracts.py holds the device to (ld_closed_forms.py): the
long-double references against independent derivations, the oracle and the reference-held known
answers; the measured r of every case; the conditions on the inputs; the regression pin of the
cancellation in the reference's algebra; and the bars themselves on float64 restatements of the
device's arithmetic (``dev64_*``: csrc/gram.h's entry and block order, csrc/moments.hip's small
algebra with explicit inverse factors), so that a bar the arithmetic cannot meet, or a mutation a
bar cannot see, shows here without a GPU.

Measured r (float64 without cancellation against long double, in |d| / |ref| / (1 + |E|)), the
largest over the sizes and d of a family: int_K at most 2.6e-15 and int_int_K1_K2 at most 9.0e-15
in every family (no cancellation to begin with).  int_K1_K2 / int_int_K1_K2_K1: mild 4.0e-15 /
7.7e-15, corr 4.8e-15 / 6.6e-15, rho9 3.3e-15 / 4.9e-15, aniso 4.6e-14 / 1.4e-14, wide4e4 2.8e-13 /
1.9e-14, wide4e6 6.1e-12 / 2.7e-13 -- in the wide families r is the points' own cancellation,
x2 - G x1 and G (x_i - x_j) formed from terms of size |x - mu| / w, about eps sqrt(cov / w^2); the
largest belong to the sizes 1 x 1 and 63 x 3, whose largest entry is itself small, so that 1 + |E|
covers little of the exponent.  Moments: r_mean at most 2.0e-15, r_Z at most 1.8e-14; t2 / t1 is
0.999992 .. 0.999997 at d = 1, 0.917 .. 0.9993 at d = 2, 0.989 .. 0.9998 at d = 3, 0.52 .. 0.71 at
d = 8.

The pin: the oracle restates the reference's algebra, Cm = W2 + 2 S - 2 S (W1 + S)^-1 S and a
Cholesky sweep over all of [[S + W1, S], [S, S + W2]], in float64.  In units of the bar, the
largest over the sizes, it errs by at most 0.22 in the mild, corr, rho9 and aniso families, by
1.17 .. 28.8 at cov / w^2 = 4e4 and by 6.7 .. 47 at 4e6.  The restated device algebra before the
fix of csrc/moments.hip: 1.1 .. 3.8 and 7.5 .. 34 at 130 x 41 and n = 65; after it at most 0.02.

Mutations of the restatements that the bars catch (run on a scratch copy): nh[k] from axis 0 for
all k -- "Gram per-entry ulps over the bound" at d = 2 .. 8; the tri route's transpose store
skipped -- "Gram entries finite and not negative" at every d; 2.0 * T replaced by
T + T' (1 + 1e-9) in Cm -- "int_int_K1_K2_K1 per-entry error over the bar"."""
import numpy as np
import pytest

import ld_closed_forms as F
from fixture_chain import build_chain, known_answers
from test_gp_sample_host import kernel_scale
from test_oracle_known_answers import _digits_ok

EPS = F.EPS
LD = F.LD
NAMES = ("int_K", "int_K1_K2", "int_int_K1_K2", "int_int_K1_K2_K1")
CANCELLING = ("int_K1_K2", "int_int_K1_K2_K1")
FAM_D = [(fam, d) for fam in F.FAMILIES for d in F.family_dims(fam)]


# ---- float64 restatements of the device's arithmetic ---------------------------------------------
def dev64_entries(xi, xj, h, w):
    """gauss_q and the entry of csrc/gram.h for the point sets xi (d x a), xj (d x b): the sum over
    the axes in order, each term (t t) nh_k, then c exp(q)."""
    d = xi.shape[0]
    nh = [-0.5 / (w[k] * w[k]) for k in range(d)]
    acc = np.zeros((xi.shape[1], xj.shape[1]))
    for k in range(d):
        t = xi[k][:, None] - xj[k][None, :]
        acc = acc + (t * t) * nh[k]
    return kernel_scale(h, w) * np.exp(np.maximum(acc, -800.0))


def dev64_gram(x, h, w, s):
    """launch_gram_sym_d: whole 64 x 64 blocks of the lower triangle with their transposes
    (gram_tri_kernel) where n % 64 == 0, every entry on its own (gram_sym_kernel) otherwise."""
    n = x.shape[1]
    K = np.full((n, n), np.nan)
    if n % 64 == 0:
        for bi in range(n // 64):
            for bj in range(bi + 1):
                I, J = slice(64 * bi, 64 * bi + 64), slice(64 * bj, 64 * bj + 64)
                B = dev64_entries(x[:, I], x[:, J], h, w)
                K[I, J] = B
                if bi != bj:
                    K[J, I] = B.T
    else:
        K[:, :] = dev64_entries(x, x, h, w)
    K[np.diag_indices(n)] += s * s
    return K


def _inv_lower(Lf):
    from scipy.linalg import solve_triangular
    return solve_triangular(Lf, np.eye(Lf.shape[0]), lower=True)


def _form(Z, Linv, logdet):
    """gauss_form_eval: logc - |Linv z|^2 / 2."""
    Y = np.tril(Linv) @ Z
    return -0.5 * (Linv.shape[0] * np.log(2.0 * np.pi) + logdet) - 0.5 * np.sum(Y * Y, axis=0)


def _fill(C):
    Lf = np.linalg.cholesky(C)
    return _inv_lower(Lf), 2.0 * np.sum(np.log(np.diag(Lf)))


def dev64_cond_cov(w, WSinv):
    """cond_cov of csrc/moments.hip."""
    W = np.diag(w * w)
    T = W - W @ WSinv @ W
    return 0.5 * (T + T.T)


def dev64_int_K(x, h, w, mu, cov):
    W, m, S = F._f64m(w, mu, cov)
    return h * h * np.exp(_form(x - m, *_fill(S + W)))


def dev64_int_K1_K2(x1, x2, h1, w1, h2, w2, mu, cov, fixed=True):
    """dev_int_K1_K2; fixed=False: the factor by a sweep over all of C2, as before the fix."""
    W1, m, S = F._f64m(w1, mu, cov)
    W2 = F._f64m(w2, mu, cov)[0]
    d, n1, n2 = x1.shape[0], x1.shape[1], x2.shape[1]
    if fixed:
        Li11, ld1 = _fill(S + W1)
        W1Sinv = Li11.T @ Li11
        Li22, ld2 = _fill(W2 + dev64_cond_cov(w1, W1Sinv))
        Linv = np.block([[Li11, np.zeros((d, d))], [-Li22 @ (S @ W1Sinv), Li22]])
        logdet = ld1 + ld2
    else:
        Linv, logdet = _fill(np.block([[S + W1, S], [S, S + W2]]))
    Z = np.vstack([np.tile(x1 - m, (1, n2)), np.repeat(x2 - m, n1, axis=1)])
    return (h1 * h1) * (h2 * h2) * np.exp(_form(Z, Linv, logdet)).reshape(n2, n1).T


def dev64_int_int_K1_K2(x, h1, w1, h2, w2, mu, cov):
    W1, m, S = F._f64m(w1, mu, cov)
    W2 = F._f64m(w2, mu, cov)[0]
    Li, ld = _fill(W1 + 2.0 * S)
    n0 = -0.5 * (x.shape[0] * np.log(2.0 * np.pi) + ld)
    Cm = W2 + S - S @ (Li.T @ Li) @ S
    return (h1 * h1) * (h2 * h2) * np.exp(n0 + _form(x - m, *_fill(Cm)))


def dev64_int_int_K1_K2_K1(x, h1, w1, h2, w2, mu, cov, fixed=True):
    """dev_iikk; fixed=False: Cm = W2 + 2 S - 2 G S, as before the fix."""
    W1, m, S = F._f64m(w1, mu, cov)
    W2 = F._f64m(w2, mu, cov)[0]
    n = x.shape[1]
    Li1, ld1 = _fill(S + W1)
    W1Sinv = Li1.T @ Li1
    G = S @ W1Sinv
    if fixed:
        Cm = W2 + 2.0 * dev64_cond_cov(w1, W1Sinv)
    else:
        Cm = W2 + 2.0 * S - 2.0 * (G @ S)
    nv = _form(x - m, Li1, ld1)
    b = G @ x
    Z = np.tile(b, (1, n)) - np.repeat(b, n, axis=1)
    f = _form(Z, *_fill(Cm)).reshape(n, n).T
    return (h1 * h1) ** 2 * (h2 * h2) * np.exp(nv[:, None] + nv[None, :] + f)


DEV64 = dict(int_K=dev64_int_K, int_K1_K2=dev64_int_K1_K2, int_int_K1_K2=dev64_int_int_K1_K2,
             int_int_K1_K2_K1=dev64_int_int_K1_K2_K1)


# ---- the references against independent derivations ---------------------------------------------
def _mild_args(d):
    h1, w1, h2, w2, mu, cov, _ = F.family_params("mild", d)
    x, x2 = F.family_points("mild", d, 65, 4), F.family_points("mild", d, 41, 3)
    return {"int_K": (x, h1, w1, mu, cov), "int_K1_K2": (x, x2, h1, w1, h2, w2, mu, cov),
            "int_int_K1_K2": (x, h1, w1, h2, w2, mu, cov),
            "int_int_K1_K2_K1": (x, h1, w1, h2, w2, mu, cov)}


@pytest.mark.parametrize("d", F.D_ALL)
def test_joint_forms_against_conditional_forms(d):
    """One joint density through one Cholesky factor against the conditional forms with explicit
    inverses (the algebra of csrc/moments.hip), both in long double: per entry, in the log."""
    for name, a in _mild_args(d).items():
        lj = F._LDF[name](*a, log=True)
        lc = getattr(F, "ldc_" + name)(*a)
        worst = float(np.max(np.abs(lj - lc) / (1 + np.abs(lj))))
        assert worst <= 1e-16, (name, d, worst)


def _relmax(a, b):
    return float(np.max(np.abs(np.asarray(a).astype(LD) - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("n", [1, 9, 63, 300])
def test_joint_forms_against_oracle_1d(oracle, n):
    """test_gpu_parity.test_device_integrals_1d's inputs and bars."""
    rs = np.random.RandomState(n)
    x = np.sort(rs.uniform(-5, 5, n))
    x2 = np.sort(rs.uniform(-6, 4, max(1, n // 2 + 3)))
    w1, w2, mu, cov = np.array([1.3]), np.array([2.0]), np.array([0.3]), np.array([[10.0]])
    o = oracle
    assert _relmax(o.int_K(x, 0.2, w1, mu, cov), F.ld_int_K(x, 0.2, w1, mu, cov)) < 1e-13
    assert _relmax(o.int_K1_K2(x, x2, 0.2, w1, 15.0, w2, mu, cov),
                   F.ld_int_K1_K2(x, x2, 0.2, w1, 15.0, w2, mu, cov)) < 1e-12
    assert _relmax(o.int_int_K1_K2_K1(x, 0.2, w1, 15.0, w2, mu, cov),
                   F.ld_int_int_K1_K2_K1(x, 0.2, w1, 15.0, w2, mu, cov)) < 1e-12
    assert _relmax(o.int_int_K1_K2(x, 0.2, w1, 15.0, w2, mu, cov),
                   F.ld_int_int_K1_K2(x, 0.2, w1, 15.0, w2, mu, cov)) < 1e-13


@pytest.mark.parametrize("d", [2, 3, 8])
def test_joint_forms_against_oracle_nd(oracle, d):
    """test_gpu_parity.test_device_integrals_nd's inputs and bars."""
    rs = np.random.RandomState(d)
    x = rs.uniform(-2, 2, (d, 70))
    x2 = rs.uniform(-2, 2, (d, 41))
    w1, w2 = rs.uniform(0.5, 1.5, d), rs.uniform(0.5, 1.5, d)
    A = rs.rand(d, d)
    cov = A.dot(A.T) + d * np.eye(d)
    mu = rs.uniform(-0.5, 0.5, d)
    o = oracle
    assert _relmax(o.int_K(x, 0.7, w1, mu, cov), F.ld_int_K(x, 0.7, w1, mu, cov)) < 1e-12
    if d <= 4:
        assert _relmax(o.int_K1_K2(x, x2, 0.7, w1, 1.2, w2, mu, cov),
                       F.ld_int_K1_K2(x, x2, 0.7, w1, 1.2, w2, mu, cov)) < 1e-11
    assert _relmax(o.int_int_K1_K2_K1(x, 0.7, w1, 1.2, w2, mu, cov),
                   F.ld_int_int_K1_K2_K1(x, 0.7, w1, 1.2, w2, mu, cov)) < 1e-11
    assert _relmax(o.int_int_K1_K2(x, 0.7, w1, 1.2, w2, mu, cov),
                   F.ld_int_int_K1_K2(x, 0.7, w1, 1.2, w2, mu, cov)) < 1e-12


def test_ld_moments_reproduce_the_known_answers(oracle):
    """E[Z] and V(Z) of the reference's notebook fixture: E[Z] to the twelve printed digits; V(Z),
    whose printed digits are those of a float64 difference of two 1e-2 terms (the file's note:
    restatements agree to about 4e-9 relative), to test_oracle_known_answers' 5e-8."""
    o = oracle
    c = build_chain(lambda x, y, h, w, s: o.gp_fit(x, y, h, w, s),
                    lambda x, h, w, L, a, xo: o.gp_predict(x, h, w, L, a, xo, want_var=False),
                    o.filter_candidates)
    exp = known_answers()["expected"]
    p_tl, p_l = (c["h1"], np.array([c["w1"]]), 0.0), (c["h2"], np.array([c["w2"]]), 0.0)
    zm, zabs = F.ld_Z_mean(c["xsc"], c["lsc"], p_l, c["mu"], c["cov"])
    assert _digits_ok(float(zm), exp["Z_mean"]["value"], exp["Z_mean"]["digits"])
    t1, t2, zv = F.ld_Z_var(c["xs"], np.log(c["ls"]), c["xsc"], c["lsc"], p_tl, p_l, c["mu"],
                            c["cov"])
    assert abs(float(zv) - exp["Z_var"]["value"]) / exp["Z_var"]["value"] < 5e-8
    assert 0 < float(t2) < float(t1)


def test_stable_cond_is_the_conditional_covariance():
    """W - W (W + S)^-1 W against the third form of the same matrix, (W^-1 + S^-1)^-1, in long
    double, S wide against W (S - S (W + S)^-1 S itself loses seven digits here even there)."""
    rs = np.random.RandomState(5)
    A = rs.rand(3, 3)
    S = 1e4 * (A @ A.T + 3 * np.eye(3))
    w = np.array([0.05, 0.07, 0.04])
    Sl, Wl = S.astype(LD), np.diag(w.astype(LD) ** 2)
    ref = F._ld_inv(F._ld_inv(Wl) + F._ld_inv(Sl))
    got = F.stable_cond(S, np.diag(w * w))
    assert float(np.max(np.abs(got - ref) / np.abs(np.diag(ref)).max())) < 16 * EPS
    assert np.array_equal(got, got.T)
    Li, _ = _fill(S + np.diag(w * w))
    got = dev64_cond_cov(w, Li.T @ Li)
    assert float(np.max(np.abs(got - ref) / np.abs(np.diag(ref)).max())) < 64 * EPS


# ---- measured r, conditions, pin ------------------------------------------------------------------
def _ratio(fam):
    return {"wide4e4": 4e4, "wide4e6": 4e6}.get(fam, 1.0)


@pytest.mark.parametrize("fam,d", FAM_D)
def test_measured_r_and_conditions_of_the_integrals(fam, d):
    """Every reference entry is a normal number, and r stays below 4 eps max(64, sqrt(cov / w^2))
    (1 + M), M the largest entry's own |log| over its h^2 factors: the yardstick's error is
    roundings of the small algebra, of the dot products (at most 3 d terms) and, in the wide
    families, of x2 - G x1 and G x_i - G x_j, whose terms are of size |x - mu| / w <=
    sqrt(cov / w^2) against a result of order one; each moves an entry by its exponent times
    itself, and the units divide by 1 + |E| only, the exponent beyond the largest entry's."""
    hh = {"int_K": lambda a: a[1] ** 2, "int_K1_K2": lambda a: (a[2] * a[4]) ** 2,
          "int_int_K1_K2": lambda a: (a[1] * a[3]) ** 2,
          "int_int_K1_K2_K1": lambda a: (a[1] * a[1] * a[3]) ** 2}
    for name in NAMES:
        worst = 0.0
        for size in F.integral_sizes(name, d):
            c = F.integral_case(fam, d, name, size)
            assert F.all_normal(c[name]), (fam, d, name, size)
            worst = max(worst, c["r"][name])
            M = abs(float(np.log(np.max(c[name]) / hh[name](c["args"]))))
            lim = 4 * EPS * max(64.0, np.sqrt(_ratio(fam))) * (1 + M)
            assert c["r"][name] <= lim, (fam, d, name, size, c["r"][name], lim)
        print("r %-8s d=%d %-17s %.2e" % (fam, d, name, worst))


@pytest.mark.parametrize("d", F.D_ALL)
def test_conditions_of_the_gram_cases(d):
    for n in F.GRAM_SIZES:
        c = F.gram_case(d, n)
        assert c["x"].shape == (d, n) and abs(c["w"][-1] / c["w"][0] - (30.0 if d > 1 else 1.0)) < 1e-9
        if n >= 63:
            print("gram d=%d n=%d normal %.3f small %.3f" % ((d, n) + F.gram_conditions(c)))
    for n1, n2 in F.CROSS_SIZES:
        if n1 >= 63:
            F.gram_conditions(F.cross_case(d, n1, n2))


@pytest.mark.parametrize("case", F.MOMENT_CASES, ids=lambda c: "d%d-%d-%d-s%g-%s" % c)
def test_conditions_of_the_moment_cases(case):
    """The long-double V(Z) is not negative; t2 / t1, r_mean and r_Z are recorded."""
    c = F.moment_case(*case)
    print("moments %s t2/t1 %.6f r_mean %.2e r_Z %.2e V(Z) %.3e t1 %.3e" % (
        case, c["ratio"], c["r_mean"], c["r_Z"], float(c["zv"]), float(c["t1"])))
    assert float(c["zv"]) >= 0.0 and float(c["t1"]) > 0.0
    assert 0.0 <= c["ratio"] <= 1.0
    assert np.isfinite(c["r_mean"]) and np.isfinite(c["r_Z"])


def _oracle_units(oracle, fam, d, name):
    """The oracle's largest error over the sizes of the GPU module, in units of each size's bar."""
    worst = 0.0
    for size in F.integral_sizes(name, d):
        c = F.integral_case(fam, d, name, size)
        got = getattr(oracle, name)(*c["args"])
        worst = max(worst, float(np.max(F.entry_units(got, c[name]))) / F.integral_bar(c["r"][name]))
    return worst


@pytest.mark.parametrize("fam,d", [(f, d) for (f, d) in FAM_D if d <= 4])
def test_reference_algebra_cancels_for_wide_measures(oracle, fam, d):
    """The regression pin.  The oracle's float64 restatement of the reference's algebra meets
    MARGIN max(r, 4 eps) in the mild families and misses it in the wide ones: the digits are lost
    in the algebra, not in float64."""
    for name in CANCELLING:
        u = _oracle_units(oracle, fam, d, name)
        print("pin %-8s d=%d %-17s %.2f bars" % (fam, d, name, u))
        if fam in F.WIDE:
            assert u > 1.0, (fam, d, name, u)
        else:
            assert u <= 1.0, (fam, d, name, u)


# ---- the bars on the restated device arithmetic ----------------------------------------------------
@pytest.mark.parametrize("d", F.D_ALL)
def test_gram_bars_on_the_restated_kernels(d):
    for n in F.GRAM_SIZES:
        c = F.gram_case(d, n)
        F.check_gram(dev64_gram(c["x"], c["h"], c["w"], c["s"]), c)
    for n1, n2 in F.CROSS_SIZES:
        c = F.cross_case(d, n1, n2)
        F.check_gram(dev64_entries(c["x1"], c["x2"], c["h"], c["w"]), c, cross=True)


@pytest.mark.parametrize("fam,d", FAM_D)
def test_integral_bars_on_the_restated_host_algebra(fam, d):
    """The fixed algebra meets every bar; the algebra before the fix misses the wide ones."""
    for name in NAMES:
        size = {"int_K": 257, "int_int_K1_K2": 257, "int_K1_K2": (130, 41),
                "int_int_K1_K2_K1": 65}[name]
        c = F.integral_case(fam, d, name, size)
        u = F.check_integral(DEV64[name](*c["args"]), c, name, symmetric=name.endswith("K1"))
        if name in CANCELLING:
            before = float(np.max(F.entry_units(DEV64[name](*c["args"], fixed=False), c[name]))) / \
                F.integral_bar(c["r"][name])
            print("restated %-8s d=%d %-17s before %.2f after %.3f bars" % (fam, d, name, before, u))
            if fam == "wide4e6":
                assert before > 1.0, (fam, d, name, before)
