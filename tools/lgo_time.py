"""Leave-group-out cross-validation on a resident fit (bq_gp_lgo, bq_gp_lgo_grad) next to
leave-one-out and to refitting without the group: python tools/lgo_time.py [N ...]

For d = 3 and N in {1024, 4096, 16384}, and three sets of groups over all N points --
  single    N singletons
  quad      a random permutation cut into groups of 4 (scattered rows)
  block64   contiguous blocks of 64
-- HIP-event times (bq_timer_*) around each call, medians of repeats after a warm-up, every call
from the state named:
  lgo_cold        lgo straight after a refit (alpha and L^-T are built first)
  lgo_warm        lgo after refit + logml_grad (alpha and L^-T are there)
  lgo_grad_cold   lgo_grad straight after a refit (and the Hessian's products stage is built)
  lgo_grad_warm   lgo_grad after refit + logml_hess (the products are there)
  loo_warm, loo_grad_warm   the leave-one-out calls from the same two states
  refit_one       wall clock of what the call replaces, for ONE group (the first): a fit of the
                  other points, predict(want_cov=True) at the group, and close()
and, from the launch profiler, the reduce-class launches of lgo_warm and lgo_grad_warm alone.
One JSON line per size and set of groups."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402


def group_sets(n):
    rs = np.random.RandomState(n)
    perm = rs.permutation(n)
    return {
        "single": [np.array([i]) for i in range(n)],
        "quad": [perm[i:i + 4] for i in range(0, n, 4)],
        "block64": [np.arange(i, min(i + 64, n)) for i in range(0, n, 64)],
    }


def run(e, n, name, groups, d=3, reps=5):
    rs = np.random.RandomState(n + d)
    x = rs.uniform(-5, 5, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    h, w, s = 1.1, np.full(d, 2.0), 0.1
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

        def lgo():
            fit.lgo(groups)

        def lgo_grad():
            fit.lgo_grad(groups)

        rows = {
            "lgo_cold": (refit, lgo),
            "lgo_warm": (with_grad, lgo),
            "lgo_grad_cold": (refit, lgo_grad),
            "lgo_grad_warm": (with_hess, lgo_grad),
            "loo_warm": (with_grad, fit.loo),
            "loo_grad_warm": (with_hess, fit.loo_grad),
        }
        for prepare, call in rows.values():  # allocations and first launches out of the way
            timed(prepare, call)
        ms = {k: [] for k in rows}
        for _ in range(reps):
            for k, (prepare, call) in rows.items():
                ms[k].append(timed(prepare, call))
        out = {"N": n, "d": d, "groups": name, "G": len(groups)}
        out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
        out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
        for k in ("lgo_warm", "lgo_grad_warm"):
            rows[k][0]()
            tl = [r for r in e.timeline(rows[k][1]) if r[0] == "reduce"]
            out[k + "_kernels_ms"] = round(sum(r[3] - r[2] for r in tl), 4)
        # what a user without the call runs, for one group
        B = groups[0]
        keep = np.setdiff1d(np.arange(n), B)
        wall = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            other = e.gp_fit(x[:, keep], y[keep], h, w, s)
            other.predict(x[:, B], want_cov=True)
            other.close()
            wall.append((time.perf_counter() - t0) * 1e3)
        out["refit_one_ms"] = round(float(np.median(wall[1:])), 3)
        return out
    finally:
        fit.close()


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096, 16384]
    e = Engine(0)
    for n in sizes:
        for name, groups in group_sets(n).items():
            print(json.dumps(run(e, n, name, groups, reps=5 if n <= 4096 else 3)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
