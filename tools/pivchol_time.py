"""The pivoted partial Cholesky of a posterior on the device (bq_gp_pivchol) next to the only
route there was before: python tools/pivchol_time.py [N ...]

For d = 3, N in {4096, 16384} x M in {4096, 16384, 65536} x q in {64, 256}, wall-clock times of
the whole call on a warm fit (block inverses resident, workspaces grown), medians of repeats after
a warm-up, the rows taken in turn within every repeat:
  pivchol  engine.Fit.pivoted_cholesky with the factor, nugget = s^2
  host     where Sigma fits (M <= 16384): predict(want_cov=True) and the same recurrence in numpy
           on the host, which touches one column of Sigma per step; beyond that there is no
           alternative and the row says so
And, from the launch profiler, the kernel time of one call split into the sweep (cross Gram,
forward row sweep, row reductions) and the steps (and per step), with the column kernels' share and the rate at
which they read W = [V | C] (8 Mp (npad + j) bytes in step j).  One JSON line per shape; the host
route's gains and variances are checked against the device's on the way, so that a wrong timing
cannot hide a wrong answer."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402

HOST_MAX_M = 16384


def host_pivchol(cov, q, nugget):
    """The recurrence of bq_gp_pivchol on a covariance in host memory (no stop: the shapes here
    keep their gains well above rounding)."""
    M = cov.shape[0]
    d = np.diag(cov).copy()
    Cf = np.zeros((M, q), order="F")
    piv, gain = np.empty(q, dtype=np.int64), np.empty(q)
    for j in range(q):
        p = int(np.argmax(d))
        c = (cov[:, p] - Cf[:, :j] @ Cf[p, :j]) / np.sqrt(d[p] + nugget)
        gain[j] = d[p]
        d -= c * c
        Cf[:, j], piv[j] = c, p
    return piv, Cf, d, gain


def kernel_split(tl, Mp, npad, q):
    """Kernel ms of one call's profiled launches (Engine.timeline rows, in launch order): the
    start of the steps is the launch whose work is 16 Mp; a step's column launch has work
    8 Mp (npad + j)."""
    ms = [r[3] - r[2] for r in tl]
    start = [i for i, r in enumerate(tl) if r[0] == "reduce" and r[4] == 16.0 * Mp][-1]
    cols = [i for i in range(start + 1, len(tl))
            if tl[i][4] == 8.0 * Mp * (npad + (i - start - 1) // 2) and (i - start) % 2 == 1]
    out = {"sweep": sum(ms[:start]), "steps": sum(ms[start:]), "per_step": sum(ms[start:]) / q}
    if len(cols) == q:
        col_ms = sum(ms[i] for i in cols)
        out["columns"] = col_ms
        out["columns_TB_per_s"] = sum(8.0 * Mp * (npad + j) for j in range(q)) / col_ms * 1e-9
    return out


def run(e, fit, n, M, q, d, s, reps):
    rs = np.random.RandomState(n + M)
    xo = np.asfortranarray(rs.uniform(-5, 5, size=(d, M)))
    nu = s * s

    def pivchol():
        return fit.pivoted_cholesky(xo, q, nugget=nu)

    def host():
        _, _, cov = fit.predict(xo, want_mean=False, want_cov=True)
        return host_pivchol(cov, q, nu)

    rows = {"pivchol": pivchol}
    piv, Cf, resid, gain = pivchol()
    assert piv.shape == (q,), (n, M, q, piv.shape)
    if M <= HOST_MAX_M:
        rows["host"] = host
        hp, hC, hres, hgain = host()
        # both run the same recurrence: equal gains to rounding (a near tie may go either way),
        # and with equal choices equal variances
        scale = float(np.max(gain))
        assert np.max(np.abs(hgain - gain)) <= 1e-9 * scale, (n, M, q)
        if np.array_equal(hp, piv):
            assert np.max(np.abs(hres - resid)) <= 1e-9 * scale, (n, M, q)

    def timed(call):
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3

    ms = {k: [] for k in rows}
    for _ in range(reps):
        for k, call in rows.items():
            ms[k].append(timed(call))
    out = {"N": n, "M": M, "q": q, "d": d}
    out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
    out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
    if "host" in rows:
        out["host_over_pivchol"] = round(out["host_ms"] / out["pivchol_ms"], 2)
    else:
        out["host"] = "no alternative"
    Mp, npad = (M + 63) // 64 * 64, (n + 63) // 64 * 64
    try:
        split = kernel_split(e.timeline(pivchol), Mp, npad, q)
        out["pivchol_kernels_ms"] = {k: round(v, 4) for k, v in split.items()}
    except Exception as err:  # the profiler's table is finite: the timings above stand without it
        out["pivchol_kernels_ms"] = "unavailable: %s" % err
    return out


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [4096, 16384]
    d, s = 3, 0.1
    e = Engine(0)
    for n in sizes:
        rs = np.random.RandomState(n)
        x = rs.uniform(-5, 5, size=(d, n))
        y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
        fit = e.gp_fit(x, y, 1.1, np.full(d, 2.0), s)
        try:
            for M in (4096, 16384, 65536):
                for q in (64, 256):
                    reps = 5 if M <= 16384 and n <= 4096 else 3
                    print(json.dumps(run(e, fit, n, M, q, d, s, reps)), flush=True)
        finally:
            fit.close()
    e.close()


if __name__ == "__main__":
    main()
