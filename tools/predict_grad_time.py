"""Gradients of the posterior at the query points (bq_gp_predict_grad) next to the prediction
itself and to the central differences they replace: python tools/predict_grad_time.py [N ...]

For N in {1024, 4096, 16384} x M in {256, 1000} x d in {1, 3}, HIP-event times (bq_timer_*) around
each call on a warm fit (block inverses and alpha resident, workspaces grown), medians of repeats
after a warm-up, the rows taken in turn within every repeat:
  predict      mean + variance (bq_gp_predict)
  grad_full    mean, variance and both gradients: predict + one backward row sweep + one launch
  grad_mean    mean and its gradient, the route without a sweep: one launch
  diff         what grad_full replaces: the 2 d mean + variance predictions of a central difference
  diff_mean    what grad_mean replaces: the 2 d mean-only predictions of a central difference
and, from the launch profiler, the kernel time of grad_full by class, its reduce-class launches
(the row reductions and predict_grad_kernel) apart.  One JSON line per shape; the differences'
results are checked against the closed form on the way, so that a wrong timing cannot hide a
wrong answer."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402


def run(e, n, M, d, reps=5):
    rs = np.random.RandomState(n + d)
    x = rs.uniform(-5, 5, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    h, w, s = 1.1, np.full(d, 0.1 if d == 1 else 2.0), 0.1
    xo = np.asfortranarray(rs.uniform(-5, 5, size=(d, M)))
    step = 1e-5 * 5.0
    shifted = []
    for k in range(d):
        e_k = np.zeros((d, 1))
        e_k[k] = step
        shifted += [np.asfortranarray(xo + e_k), np.asfortranarray(xo - e_k)]
    fit = e.gp_fit(x, y, h, w, s)
    try:
        def diff():
            return [fit.predict(p) for p in shifted]

        def diff_mean():
            return [fit.predict(p, want_var=False) for p in shifted]

        rows = {
            "predict": lambda: fit.predict(xo),
            "grad_full": lambda: fit.predict_grad(xo),
            "grad_mean": lambda: fit.predict_grad(xo, want_var=False),
            "diff": diff,
            "diff_mean": diff_mean,
        }

        def timed(call):
            e.timer_start()
            call()
            return e.timer_stop_ms()

        for call in rows.values():  # allocations, alpha and first launches out of the way
            timed(call)
        # the two ways agree (central differences: h^2 |f'''| / 6 + eps |f| / h)
        _, _, dmean, dvar = fit.predict_grad(xo)
        fd = diff()
        for k in range(d):
            fm = (fd[2 * k][0] - fd[2 * k + 1][0]) / (2 * step)
            fv = (fd[2 * k][1] - fd[2 * k + 1][1]) / (2 * step)
            assert np.max(np.abs(fm - dmean[k])) <= 1e-4 * (1 + np.max(np.abs(dmean[k]))), (n, M, d, k)
            assert np.max(np.abs(fv - dvar[k])) <= 1e-4 * (1 + np.max(np.abs(dvar[k]))), (n, M, d, k)
        ms = {k: [] for k in rows}
        for _ in range(reps):
            for k, call in rows.items():
                ms[k].append(timed(call))
        out = {"N": n, "M": M, "d": d}
        out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
        out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
        tl = e.timeline(rows["grad_full"])
        by = {}
        for r in tl:
            by[r[0]] = by.get(r[0], 0.0) + (r[3] - r[2])
        out["grad_full_kernels_ms"] = {k: round(v, 4) for k, v in sorted(by.items())}
        out["grad_full_launches"] = len(tl)
        return out
    finally:
        fit.close()


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096, 16384]
    e = Engine(0)
    for n in sizes:
        for M in (256, 1000):
            for d in (1, 3):
                print(json.dumps(run(e, n, M, d, reps=5 if n <= 4096 else 3)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
