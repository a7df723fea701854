"""Square-root-warped Bayesian quadrature on the device (bq_gp_sqintegral, bq_gp_sqdesign) next to
the routes that were there before: python tools/sqintegral_time.py [N ...]

For d = 3 and N in {4096, 16384}, wall-clock times of the whole call on a warm fit (block
inverses and alpha resident, workspaces grown), medians of repeats after a warm-up.  Once per N:
  sq_integral_warm   engine.Fit.sq_integral with its state there (nothing is launched)
  sq_integral_fresh  the same with another measure each time: the producer (two pair sums over
                     n x n, one forward sweep, three reductions, one read-back)
  refit              the yardstick for "what a call may cost"
  host               the route available before: Engine.int_K1_K2 and Engine.int_int_K1_K2_K1 to
                     host matrices, then alpha, W alpha, the bilinear form and one solve in numpy
Per A in {4096, 16384, 65536} at q = 64: engine.Fit.sq_integral_design and
engine.Fit.integral_design on the same points, alternating back to back (sq, z, z, sq in every
repeat), both states resident.  The steps are the same kernels: the difference should be the one
pair-sum launch over A x N, whose kernel time comes from the launch profiler (the launch whose
work is A N pairs), with its pairs per second; the kernel times of both calls are summed too, so
that a difference on the host shows.  One JSON line per row; the host route's numbers are checked
against the device's on the way, so that a wrong timing cannot hide a wrong answer."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def measure(d):
    return np.zeros(d), np.asfortranarray(4.0 * np.eye(d) + 1.0)


def stats(ms):
    out = {k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()}
    out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
    return out


def integral_rows(e, fit, x, h, w, n, d, s, reps=7):
    mu, cov = measure(d)
    keys = iter(range(1, 10 ** 6))

    def fresh():
        return fit.sq_integral(mu + 1e-3 * next(keys), cov)

    def host(scales=False):
        W = e.int_K1_K2(x, x, h, w, h, w, mu, cov)
        Q = e.int_int_K1_K2_K1(x, h, w, h, w, mu, cov)
        alpha = fit.alpha()
        r = W @ alpha
        bb = float(r @ fit.solve(r))
        res = (float(alpha @ r), float(alpha @ (Q @ alpha)) - bb)
        if scales:  # the sizes of the terms that both sums cancel among
            a = np.abs(alpha)
            res += (float(a @ (W @ a)), float(a @ (Q @ a)) + bb)
        return res

    sq, var = fit.sq_integral(mu, cov)
    fresh()
    hsq, hvar, ssq, svar = host(scales=True)
    # the same numbers by the other route, relative to the terms they are sums of
    assert abs(hsq - sq) <= 1e-9 * ssq, (n, hsq, sq, ssq)
    assert abs(hvar - var) <= 1e-9 * svar, (n, hvar, var, svar)
    ms = {"sq_integral_warm": [], "sq_integral_fresh": [], "refit": [], "host": []}
    for _ in range(reps):
        ms["sq_integral_fresh"].append(timed(fresh))
    fit.sq_integral(mu, cov)  # (the state holds one measure: the warm row in a loop of its own)
    for _ in range(reps):
        ms["sq_integral_warm"].append(timed(lambda: fit.sq_integral(mu, cov)))
    for _ in range(3):
        ms["refit"].append(timed(lambda: fit.refit(h, w, s)))
        fit.alpha()  # (the block inverses and alpha back, as the other rows found them)
    for _ in range(2 if n <= 4096 else 1):
        ms["host"].append(timed(host))
    out = {"N": n, "d": d, "sq": sq, "var": var}
    out.update(stats(ms))
    try:
        tl = e.timeline(fresh)
        pair = [t[3] - t[2] for t in tl if t[0] == "reduce" and t[4] == float(n) * n]
        out["fresh_kernels_ms"] = round(sum(t[3] - t[2] for t in tl), 4)
        out["fresh_pair_sums_ms"] = [round(p, 4) for p in pair]
        out["fresh_pairs_per_s"] = [round(float(n) * n / p * 1e3, 0) for p in pair]
    except Exception as err:  # the profiler's table is finite: the timings above stand without it
        out["fresh_kernels_ms"] = "unavailable: %s" % err
    return out


def design_row(e, fit, n, A, q, d, s, reps):
    rs = np.random.RandomState(n + A)
    xc = np.asfortranarray(rs.uniform(-5, 5, size=(d, A)))
    mu, cov = measure(d)
    nu = s * s
    rows = {"sqdesign": lambda: fit.sq_integral_design(xc, q, mu, cov, nugget=nu),
            "zdesign": lambda: fit.integral_design(xc, q, mu, cov, nugget=nu)}
    piv, gain, zvar0 = rows["sqdesign"]()[:3]
    assert piv.shape == (q,), (n, A, q, piv.shape)
    rows["zdesign"]()
    ms = {k: [] for k in rows}
    for _ in range(reps):
        for k in ("sqdesign", "zdesign", "zdesign", "sqdesign"):
            ms[k].append(timed(rows[k]))
    out = {"N": n, "A": A, "q": q, "d": d}
    out.update(stats(ms))
    out["sqdesign_minus_zdesign_ms"] = round(out["sqdesign_ms"] - out["zdesign_ms"], 3)
    out["var_left"] = round(float((zvar0 - gain.sum()) / zvar0), 4)
    try:
        tl = e.timeline(rows["sqdesign"])
        pair = [t[3] - t[2] for t in tl if t[0] == "reduce" and t[4] == float(A) * n]
        out["sqdesign_kernels_ms"] = round(sum(t[3] - t[2] for t in tl), 4)
        out["zdesign_kernels_ms"] = round(sum(t[3] - t[2] for t in e.timeline(rows["zdesign"])), 4)
        if len(pair) == 1:
            out["pair_sum_ms"] = round(pair[0], 4)
            out["pairs_per_s"] = round(float(A) * n / pair[0] * 1e3, 0)
    except Exception as err:
        out["sqdesign_kernels_ms"] = "unavailable: %s" % err
    return out


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [4096, 16384]
    d, s = 3, 0.1
    e = Engine(0)
    for n in sizes:
        rs = np.random.RandomState(n)
        x = np.asfortranarray(rs.uniform(-5, 5, size=(d, n)))
        l = np.exp(-0.5 * np.sum(x * x, axis=0) / 3.0 ** 2) + 0.05 + 0.01 * rs.rand(n)
        y = np.sqrt(2.0 * (l - 0.8 * l.min()))
        h, w = 1.1, np.full(d, 2.0)
        fit = e.gp_fit(x, y, h, w, s)
        try:
            print(json.dumps(integral_rows(e, fit, x, h, w, n, d, s)), flush=True)
            for A in (4096, 16384, 65536):
                reps = 6 if A <= 16384 and n <= 4096 else 3
                print(json.dumps(design_row(e, fit, n, A, 64, d, s, reps)), flush=True)
        finally:
            fit.close()
    e.close()


if __name__ == "__main__":
    main()
