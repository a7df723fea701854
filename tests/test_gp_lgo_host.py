"""CPU tests of the leave-group-out host plumbing: the formulas themselves in numpy (the gradient
against central differences of the value, the value against refits of the points outside each
group), gp.GP.clusters / lgo / log_lgo / dloglgo_dtheta (memoisation, invalidation) and
gp.GP.fit_MLII(objective="lgo", groups=...), over the oracle-backed engine double with a numpy
LGO -- and the reason the call exists, on clustered samples."""
import numpy as np
import pytest

from test_gp_loo_host import LooEngineDouble, LooFitDouble, numpy_loo, numpy_loo_grad, _data, _data2

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def _pieces(o, x, y, h, w, s):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    w = np.atleast_1d(np.asarray(w, dtype=np.float64))
    n = x.shape[1]
    L, a, _ = o.gp_fit(x, y, h, w, s)
    return x, w, o.cho_solve(L, np.eye(n)), a


def numpy_lgo(o, x, y, h, w, s, groups):
    """(mean, var, logpred, total): Sigma_B = (P_BB)^-1, r_B = Sigma_B a_B."""
    y = np.asarray(y, dtype=np.float64)
    _, _, P, a = _pieces(o, x, y, h, w, s)
    mean, var, lp = [], [], []
    for B in groups:
        B = np.asarray(B, dtype=np.int64)
        PBB = P[np.ix_(B, B)]
        S = np.linalg.inv(PBB)
        r = S @ a[B]
        mean.append(y[B] - r)
        var.append(np.diag(S))
        lp.append(0.5 * np.linalg.slogdet(PBB)[1] - 0.5 * a[B] @ r - len(B) * HALF_LOG_2PI)
    return np.concatenate(mean), np.concatenate(var), np.array(lp), float(np.sum(lp))


def numpy_lgo_grad(o, x, y, h, w, s, groups):
    """(total, [d/dh, d/dw_1 .. d/dw_d, d/ds]) with every matrix explicit:
    sum_B r_B.v_p - 1/2 r_B^T M_p r_B - 1/2 tr(Sigma_B M_p), v_p = (P D_p a)_B, M_p = (P D_p P)_BB."""
    x, w, P, a = _pieces(o, x, y, h, w, s)
    d, n = x.shape
    K0 = o.gram(x, h, w, 0.0)
    D1 = [2.0 * K0 / h]
    for j in range(d):
        r2 = (x[j][:, None] - x[j][None, :]) ** 2
        D1.append(K0 * (r2 / w[j] ** 3 - 1.0 / w[j]))
    D1.append(2.0 * s * np.eye(n))
    g = np.zeros(d + 2)
    for p, D in enumerate(D1):
        v, M = P @ (D @ a), P @ D @ P
        for B in groups:
            B = np.asarray(B, dtype=np.int64)
            S = np.linalg.inv(P[np.ix_(B, B)])
            r, MB = S @ a[B], M[np.ix_(B, B)]
            g[p] += r @ v[B] - 0.5 * r @ MB @ r - 0.5 * np.trace(S @ MB)
    return numpy_lgo(o, x, y, h, w, s, groups)[3], g


class LgoFitDouble(LooFitDouble):
    def lgo(self, groups):
        self._live()
        self.calls.append("lgo")
        return numpy_lgo(self.o, self.x, self.y, self.h, self.w, self.s, groups)

    def lgo_grad(self, groups):
        self._live()
        self.calls.append("lgo_grad")
        return numpy_lgo_grad(self.o, self.x, self.y, self.h, self.w, self.s, groups)


class LgoEngineDouble(LooEngineDouble):
    def gp_fit(self, x, y, h, w, s=0.0):
        return LgoFitDouble(self.o, x, y, h, w, s)


@pytest.fixture
def gpm(oracle):
    from bayesian_quadrature_amd import engine as eng_mod
    from bayesian_quadrature_amd import gp
    saved = dict(eng_mod._engines)
    eng_mod._engines.clear()
    eng_mod.set_engine(LgoEngineDouble(oracle), 0)
    yield gp
    eng_mod._engines.clear()
    eng_mod._engines.update(saved)


def _groups(n, seed, cover=True):
    """A random permutation cut into sizes 1 .. 7 (cover=False: of two thirds of the points)."""
    rs = np.random.RandomState(seed)
    perm = rs.permutation(n)[: n if cover else 2 * n // 3]
    out, i = [], 0
    while i < len(perm):
        b = rs.randint(1, 8)
        out.append(perm[i:i + b])
        i += b
    return out


@pytest.mark.parametrize("two_d", [False, True])
def test_numpy_lgo_gradient_matches_central_difference_of_the_value(oracle, two_d):
    if two_d:
        x, y = _data2()
        th = np.array([1.2, 0.8, 1.1, 0.2])
    else:
        x, y = _data()
        th = np.array([1.2, 0.8, 0.2])
    groups = _groups(len(y), 5, cover=not two_d)
    total, g = numpy_lgo_grad(oracle, x, y, th[0], th[1:-1], th[-1], groups)
    assert g.shape == th.shape
    assert total == numpy_lgo(oracle, x, y, th[0], th[1:-1], th[-1], groups)[3]
    for c in range(len(th)):
        e = np.zeros(len(th))
        e[c] = 1e-5 * th[c]
        v = [numpy_lgo(oracle, x, y, t[0], t[1:-1], t[-1], groups)[3] for t in (th + e, th - e)]
        fd = (v[0] - v[1]) / (2 * e[c])
        assert abs(fd - g[c]) <= 1e-5 * (1 + abs(g[c])), (c, fd, g[c])


def test_numpy_lgo_matches_refits_of_the_points_outside_each_group(oracle):
    """The check that does not share the formula: every group predicted by a fit of the rest."""
    x, y = _data(n=30)
    h, w, s = 1.2, 0.8, 0.2
    groups = _groups(len(y), 6, cover=False)
    mean, var, lp, total = numpy_lgo(oracle, x, y, h, w, s, groups)
    K = oracle.gram(x[None, :], h, np.array([w]), s)
    t = 0
    for q, B in enumerate(groups):
        o = np.setdiff1d(np.arange(len(y)), B)
        sol = np.linalg.solve(K[np.ix_(o, o)], np.column_stack([y[o], K[np.ix_(o, B)]]))
        m = K[np.ix_(B, o)] @ sol[:, 0]
        cov = K[np.ix_(B, B)] - K[np.ix_(B, o)] @ sol[:, 1:]
        b = len(B)
        assert np.all(np.abs(mean[t:t + b] - m) <= 1e-9 * (1 + np.abs(m)))
        assert np.all(np.abs(var[t:t + b] - np.diag(cov)) <= 1e-9 * np.diag(cov))
        e = y[B] - m
        ref = -0.5 * np.linalg.slogdet(cov)[1] - 0.5 * e @ np.linalg.solve(cov, e) \
            - b * HALF_LOG_2PI
        assert abs(lp[q] - ref) <= 1e-8 * (1 + abs(ref))
        t += b
    assert t == len(mean) and total == float(np.sum(lp))


def test_numpy_lgo_of_singletons_is_loo_and_of_everything_is_the_marginal_likelihood(oracle):
    x, y = _data(n=40)
    h, w, s = 1.2, 0.8, 0.2
    one = [[i] for i in range(len(y))]
    got, ref = numpy_lgo(oracle, x, y, h, w, s, one), numpy_loo(oracle, x, y, h, w, s)
    assert all(np.allclose(a, b, rtol=1e-10, atol=0) for a, b in zip(got, ref))
    assert np.allclose(numpy_lgo_grad(oracle, x, y, h, w, s, one)[1],
                       numpy_loo_grad(oracle, x, y, h, w, s)[1], rtol=1e-9, atol=1e-9)
    everything = [np.arange(len(y))]
    _, _, logml = oracle.gp_fit(x[None, :], y, h, np.array([w]), s)
    mean, var, lp, total = numpy_lgo(oracle, x, y, h, w, s, everything)
    assert abs(total - logml) <= 1e-9 * abs(logml)
    assert np.allclose(mean, 0.0, atol=1e-9)  # the prior


def test_numpy_lgo_gradient_has_no_noise_entry_without_noise(oracle):
    x, y = _data(n=20)
    assert numpy_lgo_grad(oracle, x, y, 1.2, 0.05, 0.0, _groups(20, 1))[1][-1] == 0.0


def test_clusters_split_at_the_gaps_and_cut_at_64(gpm):
    rs = np.random.RandomState(2)
    # 150 points 1e-3 apart, a pair, a triple and four loners, shuffled
    x = np.concatenate([5.0 + 1e-3 * np.arange(150), [1.0, 1.005], [2.0, 2.009, 2.018],
                        [-3.0, -1.0, 3.0, 4.0]])
    perm = rs.permutation(len(x))
    x = x[perm]
    g = gpm.GP(gpm.GaussianKernel(1.0, 1.0), x, np.zeros(len(x)), s=0.1)
    cl = g.clusters(1e-2)
    assert sorted(len(c) for c in cl) == [1, 1, 1, 1, 2, 3, 22, 64, 64]
    assert np.array_equal(np.sort(np.concatenate(cl)), np.arange(len(x)))  # a partition
    xs = [x[c] for c in cl]
    assert all(np.all(np.diff(v) > 0) and np.all(np.diff(v) <= 1e-2) for v in xs)
    assert all(xs[i][-1] < xs[i + 1][0] for i in range(len(xs) - 1))  # in the order of x
    # neighbouring clusters are further apart than thresh, unless they are runs of one cluster
    for i in range(len(xs) - 1):
        assert xs[i + 1][0] - xs[i][-1] > 1e-2 or len(xs[i]) == 64
    assert [len(c) for c in g.clusters(0.0)] == [1] * len(x)
    assert [len(c) for c in g.clusters(100.0)] == [64, 64, 31]
    with pytest.raises(ValueError):
        g.clusters(-1.0)
    with pytest.raises(ValueError):
        g.clusters(np.nan)
    assert g._fit is None  # a host helper


def test_gp_lgo_memoisation_and_invalidation(gpm, oracle):
    x, y = _data()
    g = gpm.GP(gpm.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    groups = _groups(len(y), 9)
    other = [[0, 1], [5]]
    mean, var, lp = g.lgo(groups)
    ref = numpy_lgo(oracle, x, y, 1.2, 0.8, 0.2, groups)
    assert all(np.array_equal(a, b) for a, b in zip((mean, var, lp), ref[:3]))
    assert g.log_lgo(groups) == ref[3]
    again = g.lgo([list(B) for B in groups])  # the same groups as other objects
    assert again[0] is mean and again[1] is var and again[2] is lp
    assert g._fit.calls.count("lgo") == 1
    gr = g.dloglgo_dtheta(groups)
    assert gr.shape == (3,)
    assert np.array_equal(gr, numpy_lgo_grad(oracle, x, y, 1.2, 0.8, 0.2, groups)[1])
    assert g.dloglgo_dtheta(groups) is gr and g._fit.calls.count("lgo_grad") == 1
    # other groups: their own entry, and the first stays
    assert g.log_lgo(other) == numpy_lgo(oracle, x, y, 1.2, 0.8, 0.2, other)[3]
    assert g.lgo(groups)[2] is lp and g._fit.calls.count("lgo") == 2
    ll, lo = g.log_lh, g.log_loo
    assert g.lgo(groups)[2] is lp and g.dloglgo_dtheta(groups) is gr
    assert g.log_lh == ll and g.log_loo == lo
    assert g._fit.calls.count("lgo") == 2 and g._fit.calls.count("lgo_grad") == 1

    g.set_param("h", 1.3)
    l2, g2 = g.log_lgo(groups), g.dloglgo_dtheta(groups)
    assert l2 != ref[3] and g2 is not gr and not np.array_equal(g2, gr)
    g.set_param("h", 1.3)  # no change: the memo stays
    assert g.dloglgo_dtheta(groups) is g2
    g.s = 0.25
    assert g.log_lgo(groups) != l2 and g.dloglgo_dtheta(groups) is not g2
    g.y = y + 1.0
    l3, g3 = g.log_lgo(groups), g.dloglgo_dtheta(groups)
    assert l3 == numpy_lgo(oracle, x, y + 1.0, 1.3, 0.8, 0.25, groups)[3]
    g.append([0.1, 0.7], [0.2, 0.5])
    xa, ya = np.concatenate([x, [0.1, 0.7]]), np.concatenate([y + 1.0, [0.2, 0.5]])
    assert g.log_lgo(groups) == numpy_lgo(oracle, xa, ya, 1.3, 0.8, 0.25, groups)[3]
    g4 = g.dloglgo_dtheta(groups)
    assert g4 is not g3
    assert np.array_equal(g4, numpy_lgo_grad(oracle, xa, ya, 1.3, 0.8, 0.25, groups)[1])
    g.remove([len(ya) - 1])
    assert g.log_lgo(groups) == numpy_lgo(oracle, xa[:-1], ya[:-1], 1.3, 0.8, 0.25, groups)[3]
    assert g.dloglgo_dtheta(groups) is not g4
    for bad in ([[0.5, 1.0]], [[[0, 1]]], 3):
        with pytest.raises(ValueError):
            g.lgo(bad)


def test_fit_MLII_argument_rules(gpm):
    x, y = _data()
    g = gpm.GP(gpm.GaussianKernel(1.2, 0.8), x, y, s=0.2)
    groups = g.clusters(0.1)
    for kw in ({"objective": "kfold"}, {"objective": "kfold", "groups": groups},
               {"objective": "lgo"}, {"objective": "loo", "groups": groups},
               {"objective": "log_lh", "groups": groups}, {"groups": groups}):
        with pytest.raises(ValueError):
            g.fit_MLII(["h"], **kw)
    assert g.K.h == 1.2 and g._fit is None


def test_fit_MLII_on_lgo_uses_the_lgo_gradient_only(gpm):
    x, y = _data(n=80)
    g = gpm.GP(gpm.GaussianKernel(2.0, 0.5), x, y, s=0.3)
    groups = g.clusters(0.1)
    assert 1 < len(groups) < len(y)
    start = g.log_lgo(groups)
    res = g.fit_MLII(["h", "w", "s"], objective="lgo", groups=groups)
    calls = g._fit.calls
    assert "lgo_grad" in calls
    assert "logml_grad" not in calls and "loo_grad" not in calls and "loo" not in calls
    assert res.success and res.fun == -g.log_lgo(groups)
    assert g.log_lgo(groups) >= start
    assert np.array_equal(res.x, [g.K.h, g.K.w, g.s])
    assert np.max(np.abs(g.dloglgo_dtheta(groups) * res.x)) <= 1e-3 * len(y)


def _near_duplicate_pairs(seed=0, w_true=0.7, noise=0.02):
    """20 pairs of samples 1e-3 apart of a draw from a GP with length scale w_true, observed with
    noise of standard deviation `noise`."""
    from scipy.stats import norm
    rs = np.random.RandomState(seed)
    left = np.sort(rs.uniform(-5, 5, size=20))
    x = np.sort(np.concatenate([left, left + 1e-3]))
    K = 1.0 * norm.pdf(x[:, None] - x[None, :], scale=w_true) + 1e-10 * np.eye(len(x))
    y = np.linalg.cholesky(K) @ rs.randn(len(x)) + noise * rs.randn(len(x))
    return x, y


def test_lgo_over_the_clusters_ranks_length_scales_where_loo_is_flattered(gpm):
    """Near-duplicate samples under a model whose fixed noise level (0.01) is half the data's:
    with y_i left out, its twin 1e-3 away predicts it whatever the length scale, and a length
    scale seven times too short, which listens to the twin alone, scores higher per point under
    leave-one-out than the generating one.  Leaving the pair out together ranks them the other
    way.  (Measured on the CPU before this was written down: with these settings both
    inequalities hold for each of the seeds 0 .. 11; with the model's noise at or above the
    data's, leave-one-out ranks the two length scales correctly as well, by a small margin.)"""
    x, y = _near_duplicate_pairs()
    w_true, w_short = 0.7, 0.1
    g = gpm.GP(gpm.GaussianKernel(1.0, w_true), x, y, s=0.01)
    groups = g.clusters(1e-2)
    assert [len(c) for c in groups] == [2] * 20
    loo_true, lgo_true = g.log_loo / len(y), g.log_lgo(groups) / len(y)
    g.set_param("w", w_short)
    loo_short, lgo_short = g.log_loo / len(y), g.log_lgo(groups) / len(y)
    print("per point: loo %.4g (true) %.4g (short); lgo %.4g (true) %.4g (short)"
          % (loo_true, loo_short, lgo_true, lgo_short))
    assert loo_short > loo_true
    assert lgo_true > lgo_short
