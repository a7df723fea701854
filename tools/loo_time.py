"""Leave-one-out cross-validation on a resident fit (bq_gp_loo, bq_gp_loo_grad) next to a refit
and the log-ML Hessian: python tools/loo_time.py [N ...]

For d = 1 and N in {1024, 4096, 16384}, HIP-event times (bq_timer_*) around each call, medians of
repeats after a warm-up, every call from the state named:
  refit            new hyper-parameters
  hess_fresh       logml_hess straight after a refit (alpha, L^-T, the products, the sums)
  loo_fresh        loo straight after a refit (alpha, L^-T, the row sums)
  loo_y            loo after refit + logml_grad (alpha and L^-T are there: one read of L^-T)
  loo_grad_fresh   loo_grad straight after a refit (what hess_fresh builds, and the row sums)
  loo_grad_prod    loo_grad after refit + logml_hess (the products are there: one read of
                   Kxx^-1 and of every product)
and, from the launch profiler, the reduce-class launches of loo_y and loo_grad_prod with the
bytes they have to read (8 N^2 / 2 and 8 (d + 1) N^2) over that time.  One JSON line per size."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402


def run(e, n, d=1, reps=5):
    rs = np.random.RandomState(n + d)
    x = rs.uniform(-5, 5, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    h, w, s = 1.1, np.full(d, 0.1 if d == 1 else 2.0), 0.1
    fit = e.gp_fit(x, y, h, w, s)
    try:
        def refit():
            fit.refit(h, w, s)

        def with_grad():
            refit()
            fit.logml_grad()

        def with_hess():
            refit()
            fit.logml_hess()

        def timed(prepare, call):
            prepare()
            e.timer_start()
            call()
            return e.timer_stop_ms()

        rows = {
            "refit": (lambda: None, refit),
            "hess_fresh": (refit, fit.logml_hess),
            "loo_fresh": (refit, fit.loo),
            "loo_y": (with_grad, fit.loo),
            "loo_grad_fresh": (refit, fit.loo_grad),
            "loo_grad_prod": (with_hess, fit.loo_grad),
        }
        for prepare, call in rows.values():  # allocations and first launches out of the way
            timed(prepare, call)
        ms = {k: [] for k in rows}
        for _ in range(reps):
            for k, (prepare, call) in rows.items():
                ms[k].append(timed(prepare, call))
        out = {"N": n, "d": d}
        out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
        out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
        # the new kernels alone, and the bytes they cannot avoid over that time
        for k, nbytes in (("loo_y", 4.0 * n * n), ("loo_grad_prod", 8.0 * (d + 1) * n * n)):
            rows[k][0]()
            if k == "loo_grad_prod":
                fit.loo()
            tl = [r for r in e.timeline(rows[k][1]) if r[0] == "reduce"]
            t = sum(r[3] - r[2] for r in tl)
            out[k + "_kernels_ms"] = round(t, 4)
            out[k + "_GBps"] = round(nbytes / (t * 1e-3) / 1e9, 1) if t > 0 else None
        return out
    finally:
        fit.close()


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096, 16384]
    e = Engine(0)
    for n in sizes:
        print(json.dumps(run(e, n, reps=5 if n <= 4096 else 3)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
