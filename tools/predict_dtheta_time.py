"""Derivatives of the posterior in the hyper-parameters (bq_gp_predict_dtheta) next to the
prediction itself and to the central differences they replace:
python tools/predict_dtheta_time.py [N ...]

For N in {1024, 4096, 16384} x M in {64, 1000} x d in {1, 3}, HIP-event times (bq_timer_*) around
each call on a warm fit (block inverses, alpha and the solved vectors u, z_k resident, workspaces
grown), medians of repeats after a warm-up, the rows taken in turn within every repeat:
  predict       mean + variance (bq_gp_predict)
  dtheta_full   mean, variance and both derivatives: predict + one backward row sweep + one quad
                product per length scale + one reduction
  dtheta_mean   mean and its derivatives, the route without a sweep: one launch
  dtheta_cold   dtheta_full right after a refit: the fit's solved vectors (two 64-row sweeps), the
                block inverses and alpha are rebuilt on the way (the refit itself is not timed)
  diff          what dtheta_full replaces: the 2 (d + 2) refits + predictions of a central
                difference (bq_gp_refit_predict up to its 63 points, refit + predict beyond), and
                the refit that restores the parameters
and, from the launch profiler, the kernel time of dtheta_full by class and the rate of the d
ptheta_quad_kernel launches (2 Mp n npad flops each) against what v_mfma_f64_16x16x4 can issue.
One JSON line per shape; it also carries the worst deviation of the differences from the closed
form, over all entries and relative to 1 + the row's largest entry (the differences' own noise,
eps cond(Kxx) / step, grows with N), so that a timing cannot hide a wrong answer."""
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
    theta = np.concatenate([[h], w, [s]])
    step = 1e-5 * theta
    fit = e.gp_fit(x, y, h, w, s)
    try:
        def at(t):
            if M <= 63:
                return fit.refit_predict(t[0], t[1:-1], t[-1], xo)
            fit.refit(t[0], t[1:-1], t[-1])
            return fit.predict(xo)[:2]

        def diff():
            out = []
            for p in range(d + 2):
                e_p = np.zeros(d + 2)
                e_p[p] = step[p]
                out += [at(theta + e_p), at(theta - e_p)]
            fit.refit(h, w, s)
            return out

        def cold():
            fit.refit(h, w, s)
            e.timer_start()
            fit.predict_dtheta(xo)
            return e.timer_stop_ms()

        def timed(call):
            e.timer_start()
            call()
            return e.timer_stop_ms()

        rows = {
            "predict": lambda: timed(lambda: fit.predict(xo)),
            "dtheta_full": lambda: timed(lambda: fit.predict_dtheta(xo)),
            "dtheta_mean": lambda: timed(lambda: fit.predict_dtheta(xo, want_var=False)),
            "dtheta_cold": cold,
            # (the difference ends on a refit: the fit is warmed again, untimed, for the next rows)
            "diff": lambda: (timed(diff), fit.predict_dtheta(xo))[0],
        }
        for call in rows.values():  # allocations, cached state and first launches out of the way
            call()
        # the two ways agree (central differences: step^2 |f'''| / 6 + eps cond |f| / step)
        _, _, dmean, dvar = fit.predict_dtheta(xo)
        fd = diff()
        worst = 0.0
        for p in range(d + 2):
            fm = (fd[2 * p][0] - fd[2 * p + 1][0]) / (2 * step[p])
            fv = (fd[2 * p][1] - fd[2 * p + 1][1]) / (2 * step[p])
            worst = max(worst, np.max(np.abs(fm - dmean[p])) / (1 + np.max(np.abs(dmean[p]))),
                        np.max(np.abs(fv - dvar[p])) / (1 + np.max(np.abs(dvar[p]))))
        fit.predict_dtheta(xo)
        ms = {k: [] for k in rows}
        for _ in range(reps):
            for k, call in rows.items():
                ms[k].append(call())
        out = {"N": n, "M": M, "d": d, "diff_vs_closed_form": float("%.3g" % worst)}
        out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
        out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
        fit.predict_dtheta(xo)
        tl = e.timeline(lambda: fit.predict_dtheta(xo))
        by = {}
        for r in tl:
            by[r[0]] = by.get(r[0], 0.0) + (r[3] - r[2])
        out["dtheta_full_kernels_ms"] = {k: round(v, 4) for k, v in sorted(by.items())}
        out["dtheta_full_launches"] = len(tl)
        Mp, npad = -(-M // 64) * 64, -(-n // 64) * 64
        flops = 2.0 * Mp * n * npad
        quad = [r[3] - r[2] for r in tl if r[4] == flops]
        assert len(quad) == d, (len(quad), d)
        out["quad_ms_per_launch"] = round(float(np.median(quad)), 4)
        out["quad_tflops"] = round(flops / (float(np.median(quad)) * 1e-3) / 1e12, 2)
        return out
    finally:
        fit.close()


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096, 16384]
    e = Engine(0)
    for n in sizes:
        for M in (64, 1000):
            for d in (1, 3):
                print(json.dumps(run(e, n, M, d, reps=5 if n <= 4096 else 3)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
