"""The log-ML Hessian on a resident fit (bq_gp_logml_hess) against central differences of the
gradient: python tools/logml_hess_time.py [N ...]

For d = 1 and N in {1024, 4096}: the wall time of one logml_hess on a fit whose gradient has been
taken (L^-T is there: Kxx^-1, the product per length scale, the sums), and of the route without it,
2 (d + 2) x (refit + logml_grad) at shifted parameters.  Medians of repeats after a warm-up; the
Hessian's timeline (HIP-event times: Kxx^-1, one product per length scale, the sums).  One JSON line
per size."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402


def run(e, n, d=1, reps=5):
    rs = np.random.RandomState(n + d)
    x = rs.uniform(-5, 5, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    theta = np.concatenate([[1.1], np.full(d, 0.1 if d == 1 else 2.0), [0.1]])
    p = d + 2
    fit = e.gp_fit(x, y, theta[0], theta[1:-1], theta[-1])
    try:
        def prepare():
            fit.refit(theta[0], theta[1:-1], theta[-1])
            fit.logml_grad()

        def hess():
            prepare()
            t0 = time.perf_counter()
            H = fit.logml_hess()
            return (time.perf_counter() - t0) * 1e3, H

        def central():
            t0 = time.perf_counter()
            H = np.empty((p, p))
            for c in range(p):
                g = []
                for sgn in (1.0, -1.0):
                    t = theta.copy()
                    t[c] *= 1.0 + sgn * 1e-4
                    fit.refit(t[0], t[1:-1], t[-1])
                    g.append(fit.logml_grad())
                H[:, c] = (g[0] - g[1]) / (2e-4 * theta[c])
            return (time.perf_counter() - t0) * 1e3, H

        hess(), central()  # allocations and first launches out of the way
        th, tc = [], []
        for _ in range(reps):
            th.append(hess()[0])
            tc.append(central()[0])
        H, Hc = hess()[1], central()[1]
        prepare()
        rows = e.timeline(fit.logml_hess)
        t_h, t_c = float(np.median(th)), float(np.median(tc))
        return {"N": n, "d": d, "hess_ms": round(t_h, 3), "central_diff_ms": round(t_c, 3),
                "central_over_hess": round(t_c / t_h, 3),
                "max_rel_diff": float(np.max(np.abs(H - Hc) / (1e-300 + np.abs(H)))),
                "timeline_ms": [round(r[3] - r[2], 3) for r in rows],
                "forced_tile": os.environ.get("BQ_GEMM_TILE")}
    finally:
        fit.close()


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096]
    e = Engine(0)
    for n in sizes:
        print(json.dumps(run(e, n)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
