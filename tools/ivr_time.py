"""The greedy design that minimises the integrated posterior variance on the device (bq_gp_ivr)
next to the host route: python tools/ivr_time.py [N ...]

For d = 3, N in {4096, 16384} x R = A in {1024, 4096} x q in {1, 64}, wall-clock times of the
whole call on a warm fit (block inverses resident, workspaces grown), medians of repeats after a
warm-up, the rows taken in turn within every repeat:
  ivr   engine.Fit.ivr_design with reference points of its own, nugget = s^2
  host  predict(want_cov=True) on [xr | xc] and the same recurrence in numpy on the host
And, from the launch profiler, the kernel time of one call split into the sweep (cross Gram,
forward row sweep, row reductions), the forming of T (cross Gram and product) and the steps, with
the share of the passes over T and the rate at which they move it (8 Ap Rp bytes read in step 0,
16 Ap Rp read and written in every later step).  One JSON line per shape; the host route's gains
and variances are checked against the device's on the way, so that a wrong timing cannot hide a
wrong answer."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402


def host_ivr(cov, R, rho, q, nugget):
    """The recurrence of bq_gp_ivr on a covariance over [reference points | candidates] in host
    memory (nugget > 0, no stop: the shapes here keep their gains well above rounding)."""
    T, Scc = cov[R:, :R].copy(), cov[R:, R:]
    dc, dr = np.diag(Scc).copy(), np.diag(cov)[:R].copy()
    A = T.shape[0]
    ivar0 = rho @ dr
    Cf = np.zeros((A, q), order="F")
    piv, gain = np.empty(q, dtype=np.int64), np.empty(q)
    for t in range(q):
        score = ((T * T) @ rho) / (dc + nugget)
        p = int(np.argmax(score))
        den = np.sqrt(dc[p] + nugget)
        c = (Scc[:, p] - Cf[:, :t] @ Cf[p, :t]) / den
        u = T[p] / den
        T -= np.outer(c, u)
        dc -= c * c
        dr -= u * u
        Cf[:, t], piv[t], gain[t] = c, p, score[p]
    return piv, gain, ivar0, dr, dc


def kernel_split(tl, Ap, Rp, q):
    """Kernel ms of one call's profiled launches (Engine.timeline rows, in launch order): the
    steps begin at the launch whose work is 16 (Rp + Ap); before it the last `gram` launch begins
    the forming of T; every step records the same number of rows, the first of them its pass over
    T, with work 8 Ap Rp (step 0) or 16 Ap Rp."""
    ms = [r[3] - r[2] for r in tl]
    start = [i for i, r in enumerate(tl) if r[0] == "reduce" and r[4] == 16.0 * (Rp + Ap)][-1]
    form = [i for i in range(start) if tl[i][0] == "gram"][-1]
    per = (len(tl) - start - 1) // q
    passes = list(range(start + 1, len(tl), per)) if per * q == len(tl) - start - 1 else []
    out = {"sweep": sum(ms[:form]), "form_T": sum(ms[form:start]), "steps": sum(ms[start:]),
           "per_step": sum(ms[start:]) / q}
    if len(passes) == q and all(tl[i][4] == (16.0 if k else 8.0) * Ap * Rp
                                for k, i in enumerate(passes)):
        out["passes"] = sum(ms[i] for i in passes)
        out["pass0_TB_per_s"] = 8.0 * Ap * Rp / ms[passes[0]] * 1e-9
        if q > 1:
            later = sum(ms[i] for i in passes[1:])
            out["later_passes_TB_per_s"] = 16.0 * Ap * Rp * (q - 1) / later * 1e-9
    return out


def run(e, fit, n, R, A, q, d, s, reps):
    rs = np.random.RandomState(n + R + A)
    xr = np.asfortranarray(rs.uniform(-5, 5, size=(d, R)))
    xc = np.asfortranarray(rs.uniform(-5, 5, size=(d, A)))
    rho = np.exp(-0.5 * np.sum(xr * xr, axis=0) / 4.0)
    rho /= rho.sum()
    nu = s * s
    joint = np.asfortranarray(np.concatenate([xr, xc], axis=1))

    def ivr():
        return fit.ivr_design(xc, q, xr=xr, rho=rho, nugget=nu)

    def host():
        _, _, cov = fit.predict(joint, want_mean=False, want_cov=True)
        return host_ivr(cov, R, rho, q, nu)

    rows = {"ivr": ivr, "host": host}
    piv, gain, ivar0, rr, rc = ivr()
    assert piv.shape == (q,), (n, R, A, q, piv.shape)
    hp, hgain, hivar0, hrr, hrc = host()
    # both run the same recurrence: equal gains to rounding (a near tie may go either way), and
    # with equal choices equal variances
    assert abs(hivar0 - ivar0) <= 1e-9 * ivar0 and np.max(np.abs(hgain - gain)) <= 1e-9 * ivar0
    if np.array_equal(hp, piv):
        scale = float(max(rr.max(), rc.max()))
        assert max(np.max(np.abs(hrr - rr)), np.max(np.abs(hrc - rc))) <= 1e-9 * scale

    def timed(call):
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3

    ms = {k: [] for k in rows}
    for _ in range(reps):
        for k, call in rows.items():
            ms[k].append(timed(call))
    out = {"N": n, "R": R, "A": A, "q": q, "d": d}
    out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
    out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
    out["host_over_ivr"] = round(out["host_ms"] / out["ivr_ms"], 2)
    Ap, Rp = (A + 63) // 64 * 64, (R + 63) // 64 * 64
    try:
        split = kernel_split(e.timeline(ivr), Ap, Rp, q)
        out["ivr_kernels_ms"] = {k: round(v, 4) for k, v in split.items()}
    except Exception as err:  # the profiler's table is finite: the timings above stand without it
        out["ivr_kernels_ms"] = "unavailable: %s" % err
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
            for m in (1024, 4096):
                for q in (1, 64):
                    reps = 5 if m <= 1024 else 3
                    print(json.dumps(run(e, fit, n, m, m, q, d, s, reps)), flush=True)
        finally:
            fit.close()
    e.close()


if __name__ == "__main__":
    main()
