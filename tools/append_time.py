"""Appending observations to a resident fit (bq_gp_append) against refactoring it:
python tools/append_time.py [N ...]

For N in {1024, 4096, 16384} and k in {1, 64}, one process, everything warm: the median of
`append` + `logml` from N - k to N points (the layout holds them: no growth) and from N to N + k
(N is a multiple of 64: the layout grows, the factor is copied), by the host clock and by HIP
events; `refit` of the N-point fit and a fresh `gp_fit` of N points, measured in the same run --
the two routes an added observation took before; and, from the launch profiler's timeline of one
append, the span and the summed kernel time of the sweep's launches (trsm + gemm_panel: two per 64
columns).  One JSON line per configuration."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402


def _timed(e, fn):
    """(host ms, HIP-event ms) of fn()."""
    e.sync()
    e.timer_start()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    return host, e.timer_stop_ms()


def _median(pairs):
    a = np.median(np.array(pairs), axis=0)
    return round(float(a[0]), 4), round(float(a[1]), 4)


def run(e, n, k, reps=7):
    rs = np.random.RandomState(n + k)
    N = n + k
    dx = 10.0 / (N - 1)
    x = (np.linspace(-5, 5, N) + rs.uniform(-dx / 4, dx / 4, N))[rs.permutation(N)]
    y = np.sin(x) + 0.01 * rs.randn(N)
    h, w, s = 1.3, np.array([dx]), 1e-2

    def append_from(n0):
        """append + logml from n0 to n0 + k points on a new fit each time (untimed)."""
        out = []
        for _ in range(reps + 1):
            fit = e.gp_fit(x[:n0], y[:n0], h, w, s)
            try:
                out.append(_timed(e, lambda: (fit.append(x[n0:n0 + k], y[n0:n0 + k]), fit.logml)))
            finally:
                fit.close()
        return _median(out[1:])  # the first one grows the context's scratch

    stay = append_from(n - k)
    grow = append_from(n)
    fit = e.gp_fit(x[:n], y[:n], h, w, s)
    try:
        fit.refit(h, w, s)
        refit = _median([_timed(e, lambda: (fit.refit(h, w, s), fit.logml)) for _ in range(reps)])
    finally:
        fit.close()

    def fresh():
        f = e.gp_fit(x[:n], y[:n], h, w, s)
        f.logml
        f.close()

    fresh()
    fit_ms = _median([_timed(e, fresh) for _ in range(reps)])
    fit = e.gp_fit(x[:n - k], y[:n - k], h, w, s)
    try:
        rows = e.timeline(lambda: fit.append(x[n - k:n], y[n - k:n]))
    finally:
        fit.close()
    sweep = [r for r in rows if r[0] in ("trsm", "gemm_panel")]
    span = (max(r[3] for r in sweep) - min(r[2] for r in sweep)) if sweep else 0.0
    return {"N": n, "k": k, "append_ms": stay[0], "append_event_ms": stay[1],
            "append_grow_ms": grow[0], "append_grow_event_ms": grow[1],
            "refit_ms": refit[0], "refit_event_ms": refit[1],
            "fit_ms": fit_ms[0], "fit_event_ms": fit_ms[1],
            "refit_over_append": round(refit[0] / stay[0], 2),
            "refit_over_append_grow": round(refit[0] / grow[0], 2),
            "launches": len(rows), "sweep_launches": len(sweep),
            "sweep_span_ms_profiled": round(float(span), 4),
            "sweep_kernel_ms": round(float(sum(r[3] - r[2] for r in sweep)), 4)}


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096, 16384]
    e = Engine(0)
    for n in sizes:
        for k in (1, 64):
            print(json.dumps(run(e, n, k)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
