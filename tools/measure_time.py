"""The integral of a resident fit and its designs under a box and under mixtures of Gaussians,
next to the single Gaussian (bq_gp_integral_box / _mix, bq_gp_zdesign_box / _mix):
python tools/measure_time.py [N ...]

d = 3.  Per N in {4096, 16384}: ``integral`` with the KMEAN state computed anew -- every call asks
for a measure the fit has not seen -- for the Gaussian, the box and mixtures of 1, 4, 16 and 64
components, the six alternating inside each repeat; wall clock of the whole call, medians and
minima of the repeats after a warm-up, and from the launch profiler the kernel time of the
producer's first launch, the kernel mean on the resident points.  ``host_kk``: the host's share that
grows with the measure, kk alone (Engine.int_K_box / int_K_mix with no points).
At N = 4096, A in {4096, 16384, 65536}, q = 64: ``integral_design`` for the box and for the
16-component mixture, each alternating back to back with the Gaussian call (new, gauss, gauss, new
in every repeat; the two share the fit's one state, so every call of either row computes its state
anew), and the kernel time of the kernel mean at the A candidates.
One JSON line per row."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import BoxMeasure, Engine, GaussianMixture  # noqa: E402

D = 3


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def mixture(C, shift=0.0):
    rs = np.random.RandomState(C)
    mu = rs.uniform(-3.0, 3.0, (C, D)) + shift
    sc = rs.uniform(0.5, 2.0, C)
    cov = np.array([s * s * (0.7 * np.eye(D) + 0.3) for s in sc])
    return GaussianMixture(np.full(C, 1.0 / C), mu, cov)


def measures(shift):
    """The six measures, moved by ``shift`` so that none is the one the state holds."""
    out = {"gauss": (np.full(D, shift), np.asfortranarray(4.0 * np.eye(D) + 1.0)),
           "box": (BoxMeasure(np.full(D, -3.0 + shift), np.full(D, 3.0 + shift)),)}
    for C in (1, 4, 16, 64):
        out["mix%d" % C] = (mixture(C, shift),)
    return out


def kappa_ms(e, call, n, pick=0):
    """Kernel ms of a kernel-mean launch over n points in one call (work 8 (d + 1) n): the first
    is the producer's, on the resident points, the last a design's, on its candidates."""
    try:
        rows = [r for r in e.timeline(call) if r[4] == 8.0 * (D + 1.0) * n]
        return round(rows[pick][3] - rows[pick][2], 4) if rows else None
    except Exception as err:  # the profiler's table is finite: the wall clock stands without it
        return "unavailable: %s" % err


def state_rows(e, fit, h, w, n, reps=9):
    keys = iter(range(1, 10 ** 6))
    names = list(measures(0.0))
    for k in names:   # warm-up: every route once, buffers grown
        fit.integral(*measures(1e-3 * next(keys))[k])
    ms = {k: [] for k in names}
    for _ in range(reps):
        ms_now = measures(1e-3 * next(keys))
        for k in names:
            ms[k].append(timed(lambda: fit.integral(*ms_now[k])))
    once = measures(1e-3 * next(keys))
    for k in names:
        out = {"N": n, "d": D, "measure": k, "state_anew_ms": round(float(np.median(ms[k])), 4),
               "state_anew_min_ms": round(float(np.min(ms[k])), 4),
               "kappa_kernel_ms": kappa_ms(e, lambda: fit.integral(*once[k]), n)}
        if k != "gauss":
            m = once[k][0]
            fn = e.int_K_box if k == "box" else e.int_K_mix
            t = [timed(lambda: fn(np.zeros((D, 0)), h, w, m, want_kk=True)) for _ in range(reps)]
            out["host_kk_ms"] = round(float(np.median(t)), 4)
        warm = [timed(lambda: fit.integral(*once[k])) for _ in range(reps)]
        out["state_there_ms"] = round(float(np.median(warm)), 4)
        print(json.dumps(out), flush=True)


def design_rows(e, fit, n, s, q=64, reps=5):
    ms0 = measures(0.0)
    for A in (4096, 16384, 65536):
        xc = np.asfortranarray(np.random.RandomState(n + A).uniform(-5, 5, size=(D, A)))
        for k in ("box", "mix16"):
            rows = {"new": lambda: fit.integral_design(xc, q, *ms0[k], nugget=s * s),
                    "gauss": lambda: fit.integral_design(xc, q, *ms0["gauss"], nugget=s * s)}
            # (the two share one state: each call finds the other's and computes its own anew,
            # the same for both rows)
            piv = rows["new"]()[0]
            rows["gauss"]()
            assert piv.shape == (q,), (k, A, piv.shape)
            ms = {"new": [], "gauss": []}
            for _ in range(reps):
                for r in ("new", "gauss", "gauss", "new"):
                    ms[r].append(timed(rows[r]))
            out = {"N": n, "A": A, "q": q, "d": D, "measure": k}
            for r in ms:
                out[r + "_ms"] = round(float(np.median(ms[r])), 3)
                out[r + "_min_ms"] = round(float(np.min(ms[r])), 3)
            out["new_minus_gauss_ms"] = round(out["new_ms"] - out["gauss_ms"], 3)
            out["kappa_kernel_ms"] = {r: kappa_ms(e, rows[r], A, -1) for r in ("new", "gauss")}
            print(json.dumps(out), flush=True)


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [4096, 16384]
    s = 0.1
    e = Engine(0)
    for n in sizes:
        rs = np.random.RandomState(n)
        x = np.asfortranarray(rs.uniform(-5, 5, size=(D, n)))
        y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
        h, w = 1.1, np.full(D, 2.0)
        fit = e.gp_fit(x, y, h, w, s)
        try:
            state_rows(e, fit, h, w, n)
            if n == 4096:
                design_rows(e, fit, n, s)
        finally:
            fit.close()
    e.close()


if __name__ == "__main__":
    main()
