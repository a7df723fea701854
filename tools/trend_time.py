"""The polynomial trend of a resident fit (bq_gp_trend, bq_gp_predict_trend) next to the zero-mean
prediction and to a refit: python tools/trend_time.py [N ...]

For N in {4096, 16384}, M = 1000: d = 3 with every degree (p = 1, 4, 10: the first two ride in the
row reductions' pass over V, the third goes out as a product) and d = 8 with degree 2 (p = 45, the
product).  HIP-event times (bq_timer_*) around each call on a warm fit (block inverses, z and the
trend's state resident, workspaces grown; after the refit row they are rebuilt outside the clock),
medians of repeats after a warm-up, the rows taken in turn within every repeat:
  predict        mean + variance (bq_gp_predict)
  trend_full     mean + variance under the trend, its state resident (bq_gp_predict_trend)
  predict_mean   the mean alone, the route without a sweep
  trend_mean     the same under the trend
  refit          new hyper-parameters (bq_gp_refit): what drops the trend's state
  trend          the state anew after that refit, the block inverses rebuilt before the clock
                 starts (bq_gp_trend: basis, one 64-row sweep, sums, solve, one vector sweep)
and, from the launch profiler, the kernel time of trend_full by class with its launch count, and
the route it took.  One JSON line per shape; the two routes' means are compared on the way, so that
a wrong timing cannot hide a wrong answer."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402


def run(e, n, M, d, degree, reps=5):
    rs = np.random.RandomState(n + d)
    x = rs.uniform(-5, 5, size=(d, n))
    y = np.sin(x).sum(axis=0) - 0.1 * (x * x).sum(axis=0) + 0.1 * rs.randn(n)
    h, w, s = 1.1, np.full(d, 2.0 if d <= 3 else 4.0), 0.1
    xo = np.asfortranarray(rs.uniform(-6, 6, size=(d, M)))
    c = x.mean(axis=1)
    rho = np.max(np.abs(x - c[:, None]), axis=1)
    fit = e.gp_fit(x, y, h, w, s)
    try:
        def timed(call):
            e.timer_start()
            call()
            return e.timer_stop_ms()

        rows = {
            "predict": lambda: fit.predict(xo),
            "trend_full": lambda: fit.predict_trend(xo, degree, c, rho),
            "predict_mean": lambda: fit.predict(xo, want_var=False),
            "trend_mean": lambda: fit.predict_trend(xo, degree, c, rho, want_var=False),
            "refit": lambda: fit.refit(h, w, s),
        }
        for call in rows.values():  # allocations, alpha and first launches out of the way
            timed(call)
        fit.predict(xo)
        m_full, v_full = fit.predict_trend(xo, degree, c, rho)
        route = fit.trend_last_route()
        m_mean = fit.predict_trend(xo, degree, c, rho, want_var=False)[0]
        assert np.max(np.abs(m_full - m_mean)) <= 1e-8 * (1 + np.max(np.abs(m_full))), (n, d, degree)
        assert np.all(v_full >= fit.predict(xo)[1])
        ms = {k: [] for k in list(rows) + ["trend"]}
        for _ in range(reps):
            for k, call in rows.items():
                ms[k].append(timed(call))
            fit.predict(xo)  # the block inverses, z and alpha back, outside the clock
            fit.predict(xo, want_var=False)
            ms["trend"].append(timed(lambda: fit.trend(degree, c, rho)))
        out = {"N": n, "M": M, "d": d, "degree": degree, "p": int(fit.trend(degree, c, rho)[0].size),
               "route": route[0], "gemm_kernel": route[1]}
        out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
        out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
        for name in ("predict", "trend_full"):
            tl = e.timeline(rows[name])
            by = {}
            for r in tl:
                by[r[0]] = by.get(r[0], 0.0) + (r[3] - r[2])
            out[name + "_kernels_ms"] = {k: round(v, 4) for k, v in sorted(by.items())}
            out[name + "_launches"] = len(tl)
        return out
    finally:
        fit.close()


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [4096, 16384]
    e = Engine(0)
    for n in sizes:
        for d, degree in ((3, 0), (3, 1), (3, 2), (8, 2)):
            print(json.dumps(run(e, n, 1000, d, degree, reps=5 if n <= 4096 else 3)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
