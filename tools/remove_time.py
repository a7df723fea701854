"""Removing observations from a resident fit (bq_gp_remove) against the route there was before:
python tools/remove_time.py [N ...]

For N in {1024, 4096, 16384}, k in {1, 64} and the removed indices at the front, in the middle and
at the back of the fit, one process, everything warm: the median of `remove` + `logml` on a
resident fit of N points (a new fit each time, fitted untimed), by the host clock and by HIP
events, against `close()` + `gp_fit` of the N - k survivors + `logml`, measured in the same run and
alternating with it.  One JSON line per configuration; `refit_over_remove` below 1 is a case the
update route loses."""
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


def run(e, n, k, where, reps=5):
    rs = np.random.RandomState(n + k)
    dx = 10.0 / (n - 1)
    x = (np.linspace(-5, 5, n) + rs.uniform(-dx / 4, dx / 4, n))[rs.permutation(n)]
    y = np.sin(x) + 0.01 * rs.randn(n)
    h, w, s = 1.3, np.array([dx]), 1e-2
    first = {"front": 0, "middle": (n - k) // 2, "back": n - k}[where]
    idx = np.arange(first, first + k)
    xs, ys = np.delete(x, idx), np.delete(y, idx)
    remove, refit = [], []
    for _ in range(reps + 1):  # (the first round grows the context's scratch)
        fit = e.gp_fit(x, y, h, w, s)
        try:
            remove.append(_timed(e, lambda: (fit.remove(idx), fit.logml)))
        finally:
            fit.close()
        fit = e.gp_fit(x, y, h, w, s)
        box = []

        def old_route():
            fit.close()
            box.append(e.gp_fit(xs, ys, h, w, s))
            box[0].logml

        try:
            refit.append(_timed(e, old_route))
        finally:
            fit.close()
            for f in box:
                f.close()
    rm, rf = _median(remove[1:]), _median(refit[1:])
    fit = e.gp_fit(x, y, h, w, s)
    try:
        rows = e.timeline(lambda: fit.remove(idx))
    finally:
        fit.close()
    return {"N": n, "k": k, "where": where, "first": int(first),
            "remove_ms": rm[0], "remove_event_ms": rm[1],
            "close_fit_ms": rf[0], "close_fit_event_ms": rf[1],
            "refit_over_remove": round(rf[0] / rm[0], 2), "launches": len(rows),
            "kernel_ms": round(float(sum(r[3] - r[2] for r in rows)), 4)}


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096, 16384]
    e = Engine(0)
    for n in sizes:
        for k in (1, 64):
            for where in ("front", "middle", "back"):
                print(json.dumps(run(e, n, k, where)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
