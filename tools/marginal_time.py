"""The marginal of a resident fit next to ``predict`` at the same query count (bq_gp_marginal,
bq_gp_marginal_box): python tools/marginal_time.py [N ...]

d = 3, one kept axis.  Per N in {4096, 16384} and M in {256, 1000, 4096}: ``marginal`` with the
variance (Gaussian and box) and ``predict`` with the variance on M points, alternating back to back
inside each repeat (marginal, predict, predict, marginal); the mean-only routes the same way; wall
clock of the whole call, medians, minima and the spread (max - min) of the repeats after a warm-up.
From the launch profiler the kernel time of the cross producer (marginal_cross_kernel) beside
predict's (gram_cross_pad_kernel or gram_cross_kernel: the row of class GRAM in each call).
``today``: what a user does without the call -- ``predict`` (mean only) on M x 16 x 16
Gauss-Hermite nodes of the conditional and the weighted sum, where M x 256 points fit one call.
One JSON line per row."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import BoxMeasure, Engine  # noqa: E402

D = 3
AXES = (0,)
REPS = 7


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    v = np.asarray(v)
    return {"ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4),
            "spread_ms": round(float(v.max() - v.min()), 4)}


def gram_ms(e, call):
    """Kernel ms of the call's cross producer: its launch of class GRAM with the most work."""
    try:
        rows = [r for r in e.timeline(call) if "GRAM" in str(r[0]).upper()]
        if not rows:
            return None
        r = max(rows, key=lambda r: r[4])
        return round(r[3] - r[2], 4)
    except Exception as err:  # the profiler's table is finite: the wall clock stands without it
        return "unavailable: %s" % err


def alternate(a, b, reps=REPS):
    ta, tb = [], []
    a(), b()
    for _ in range(reps):
        ta.append(timed(a)), tb.append(timed(b)), tb.append(timed(b)), ta.append(timed(a))
    return stats(ta), stats(tb)


def today(fit, q, mu, cov):
    """predict on the 16 x 16 Gauss-Hermite nodes of the conditional of the two integrated axes
    given q, weighted and scaled by pi_S(q)."""
    t, wh = np.polynomial.hermite_e.hermegauss(16)
    wh = wh / np.sqrt(2 * np.pi)
    S, I = [0], [1, 2]
    B = cov[np.ix_(I, S)] / cov[0, 0]
    Lc = np.linalg.cholesky(cov[np.ix_(I, I)] - B @ cov[np.ix_(S, I)])
    T = np.stack(np.meshgrid(t, t, indexing="ij")).reshape(2, -1)
    W = np.outer(wh, wh).ravel()
    M = q.shape[0]
    pts = np.empty((D, M, 256))
    pts[0] = q[:, None]
    pts[1:] = (mu[I][:, None] + B * (q - mu[0])[None, :])[:, :, None] + (Lc @ T)[:, None, :]
    mean = fit.predict(np.asfortranarray(pts.reshape(D, -1)), want_var=False)[0].reshape(M, 256)
    piS = np.exp(-0.5 * (q - mu[0]) ** 2 / cov[0, 0]) / np.sqrt(2 * np.pi * cov[0, 0])
    return piS * (mean @ W)


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [4096, 16384]
    s = 0.1
    e = Engine(0)
    mu, cov = np.full(D, 0.3), np.asfortranarray(4.0 * np.eye(D) + 1.0)
    box = BoxMeasure(np.full(D, -3.0), np.full(D, 3.0))
    for n in sizes:
        rs = np.random.RandomState(n)
        x = np.asfortranarray(rs.uniform(-5, 5, size=(D, n)))
        y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
        h, w = 1.1, np.full(D, 2.0)
        fit = e.gp_fit(x, y, h, w, s)
        try:
            for M in (256, 1000, 4096):
                q = rs.uniform(-3.0, 3.0, M)
                xo = np.asfortranarray(rs.uniform(-3.0, 3.0, (D, M)))
                calls = {
                    "marginal": lambda: fit.marginal(q, AXES, mu, cov),
                    "marginal_box": lambda: fit.marginal(q, AXES, box),
                    "predict": lambda: fit.predict(xo),
                    "marginal_mean": lambda: fit.marginal(q, AXES, mu, cov, want_var=False),
                    "predict_mean": lambda: fit.predict(xo, want_var=False),
                }
                out = {"N": n, "M": M, "d": D}
                out["marginal"], out["predict"] = alternate(calls["marginal"], calls["predict"])
                out["marginal_box"], out["predict_b"] = alternate(calls["marginal_box"],
                                                                  calls["predict"])
                out["marginal_mean"], out["predict_mean"] = alternate(calls["marginal_mean"],
                                                                      calls["predict_mean"])
                out["marginal_over_predict"] = round(out["marginal"]["ms"] / out["predict"]["ms"], 3)
                out["cross_kernel_ms"] = {k: gram_ms(e, calls[k])
                                          for k in ("marginal", "marginal_box", "predict")}
                if M * 256 <= 1 << 18:
                    tt = [timed(lambda: today(fit, q, mu, cov)) for _ in range(REPS)]
                    out["today"] = stats(tt)
                    j = fit.marginal(q, AXES, mu, cov, want_var=False)[0]
                    out["today_against_marginal"] = float(
                        np.max(np.abs(today(fit, q, mu, cov) - j)) / np.max(np.abs(j)))
                print(json.dumps(out), flush=True)
        finally:
            fit.close()
    e.close()


if __name__ == "__main__":
    main()
