"""The log-ML gradient on a resident fit (bq_gp_logml_grad) against the refits a central difference
takes: python tools/logml_grad_time.py [N ...]

For N in {1024, 2048, 4096, 16384} and d in {1, 8}: the refit's wall time, the gradient's wall time
right after a refit (triangular inverse + fused product) and on a repeat (the inverse kept: the
fused product alone), the 2p + 1 refits of a central difference (p = d + 2), and the fused
kernel's HIP-event time and TFLOP/s on its npad^3 / 3 flops (the launch profiler's timeline:
the product is the gradient's second-to-last launch, the finalize its last).  One JSON line per
configuration."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402

PEAK_TFLOPS = 78.6  # fp64 matrix peak of the MI355X


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run(e, n, d, reps=5):
    rs = np.random.RandomState(n + d)
    x = rs.uniform(-5, 5, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    h, s = 1.1, 0.1
    w = np.full(d, 0.1 if d == 1 else 2.0)
    fit = e.gp_fit(x, y, h, w, s)
    try:
        fit.logml_grad()  # allocations and first launches out of the way
        refit = _median_ms(lambda: fit.refit(h, w, s), reps)

        def grad_after_refit():
            fit.refit(h, w, s)
            t0 = time.perf_counter()
            fit.logml_grad()
            return (time.perf_counter() - t0) * 1e3

        grad = float(np.median([grad_after_refit() for _ in range(reps)]))
        grad_repeat = _median_ms(fit.logml_grad, reps)
        fit.refit(h, w, s)
        rows = e.timeline(fit.logml_grad)
        prod = rows[-2]
        kern_ms = prod[3] - prod[2]
        npad = (n + 63) // 64 * 64
        tflops = npad ** 3 / 3.0 / (kern_ms * 1e-3) / 1e12
        p = d + 2
        return {"N": n, "d": d, "refit_ms": round(refit, 3), "grad_ms": round(grad, 3),
                "grad_repeat_ms": round(grad_repeat, 3),
                "central_diff_ms": round((2 * p + 1) * refit, 3),
                "grad_over_refit": round(grad / refit, 3),
                "fused_kernel_ms": round(kern_ms, 3), "fused_tflops": round(tflops, 2),
                "fused_frac_peak": round(tflops / PEAK_TFLOPS, 3), "launches": len(rows),
                "forced_tile": os.environ.get("BQ_GEMM_TILE")}
    finally:
        fit.close()


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1024, 2048, 4096, 16384]
    e = Engine(0)
    for n in sizes:
        for d in (1, 8):
            print(json.dumps(run(e, n, d)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
