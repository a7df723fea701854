"""The greedy design that lowers the variance of the integral on the device (bq_gp_zdesign) next
to the other designs: python tools/zdesign_time.py [N ...]

For d = 3, N in {4096, 16384} x A in {4096, 16384, 65536} at q = 64, and q in {1, 256} at
N = 4096, A = 16384, wall-clock times of the whole call on a warm fit (block inverses resident,
workspaces grown, the kernel means of the measure resident), medians of repeats after a warm-up,
the new route and its yardstick alternating back to back (zdesign, pivchol, pivchol, zdesign in
every repeat), the other rows after them in loops of their own:
  zdesign  engine.Fit.integral_design, nugget = s^2
  pivchol  engine.Fit.pivoted_cholesky on the same points and q without the factor: the yardstick,
           whose code this route shares (the sweep and the column kernel)
  ivr      engine.Fit.ivr_design with R = 4096 reference points drawn from the measure, where T
           fits (A R <= 2^28 entries)
  host     where Sigma fits (A <= 16384): predict(want_cov=True), u0 from int_K and solve, and the
           same recurrence in numpy on the host
Once per N: a refit, a single-vector solve, and ``integral`` with its state there (one dot
product) and with another measure (the producer: int_K, one forward sweep, one reduction).
From the launch profiler, the kernel time of one zdesign call split into the sweep (cross Gram,
forward row sweep, row reductions, kappa, V b; the row reductions and V b also on their own) and
the steps, with the column kernels' share and the rate at which they read W = [V | C]
(8 Ap (npad + t) bytes in step t).  One JSON line per
shape; the host route's gains are checked against the device's on the way, so that a wrong timing
cannot hide a wrong answer."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402

HOST_MAX_A = 16384
IVR_R = 4096
IVR_MAX_CELLS = 2 ** 28


def host_zdesign(cov, u0, q, nugget):
    """The recurrence of bq_gp_zdesign on a covariance in host memory (nugget > 0, no stop: the
    shapes here keep their gains well above rounding)."""
    A = cov.shape[0]
    dc, u = np.diag(cov).copy(), u0.copy()
    Cf = np.zeros((A, q), order="F")
    piv, gain = np.empty(q, dtype=np.int64), np.empty(q)
    for t in range(q):
        score = u * u / (dc + nugget)
        p = int(np.argmax(score))
        den = np.sqrt(dc[p] + nugget)
        c = (cov[:, p] - Cf[:, :t] @ Cf[p, :t]) / den
        u -= c * (u[p] / den)
        dc -= c * c
        Cf[:, t], piv[t], gain[t] = c, p, score[p]
    return piv, gain, u, dc


def kernel_split(tl, Ap, npad, q):
    """Kernel ms of one call's profiled launches (Engine.timeline rows, in launch order): the
    start of the steps is the launch whose work is 48 Ap, the two before it are the prediction's
    row reductions and the pass that forms V b (8 Ap npad bytes each); a step's column launch has
    work 8 Ap (npad + t)."""
    ms = [r[3] - r[2] for r in tl]
    start = [i for i, r in enumerate(tl) if r[0] == "reduce" and r[4] == 48.0 * Ap][-1]
    cols = [i for i in range(start + 1, len(tl))
            if tl[i][4] == 8.0 * Ap * (npad + (i - start - 1) // 2) and (i - start) % 2 == 1]
    out = {"sweep": sum(ms[:start]), "steps": sum(ms[start:]), "per_step": sum(ms[start:]) / q}
    # (the kernel mean at the candidates has a row of its own between the two, work 8 (d + 1) A)
    big = [i for i in range(start) if tl[i][4] == 8.0 * Ap * npad]
    if len(big) >= 2 and big[-1] == start - 1:
        out["rowdot"], out["vb"] = ms[big[-2]], ms[big[-1]]
        out["vb_TB_per_s"] = 8.0 * Ap * npad / ms[big[-1]] * 1e-9
    if len(cols) == q:
        col_ms = sum(ms[i] for i in cols)
        out["columns"] = col_ms
        out["columns_TB_per_s"] = sum(8.0 * Ap * (npad + t) for t in range(q)) / col_ms * 1e-9
    return out


def pivchol_split(tl, Ap, q):
    """The same split of a pivoted_cholesky call: its steps begin at the launch whose work is
    16 Ap."""
    ms = [r[3] - r[2] for r in tl]
    start = [i for i, r in enumerate(tl) if r[0] == "reduce" and r[4] == 16.0 * Ap][-1]
    return {"sweep": sum(ms[:start]), "steps": sum(ms[start:]), "per_step": sum(ms[start:]) / q}


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def measure(d):
    return np.zeros(d), np.asfortranarray(4.0 * np.eye(d) + 1.0)


def run(e, fit, x, h, w, n, A, q, d, s, reps):
    rs = np.random.RandomState(n + A)
    xc = np.asfortranarray(rs.uniform(-5, 5, size=(d, A)))
    mu, cov = measure(d)
    xr = np.asfortranarray(rs.multivariate_normal(mu, cov, size=IVR_R).T)
    rho = np.full(IVR_R, 1.0 / IVR_R)
    nu = s * s

    def zdesign():
        return fit.integral_design(xc, q, mu, cov, nugget=nu)

    def pivchol():
        return fit.pivoted_cholesky(xc, q, nugget=nu, want_factor=False)

    def ivr():
        return fit.ivr_design(xc, q, xr=xr, rho=rho, nugget=nu)

    def host():
        _, _, sig = fit.predict(xc, want_mean=False, want_cov=True)
        wts = fit.solve(e.int_K(x, h, w, mu, cov))
        u0 = e.int_K(xc, h, w, mu, cov) - e.gram_cross(xc, x, h, w) @ wts
        return host_zdesign(sig, u0, q, nu)

    rows = {"zdesign": zdesign, "pivchol": pivchol}
    piv, gain, zvar0, ru, rc = zdesign()
    assert piv.shape == (q,), (n, A, q, piv.shape)
    pivchol()
    Ap = (A + 63) // 64 * 64
    if Ap * IVR_R <= IVR_MAX_CELLS:
        rows["ivr"] = ivr
        ivr()
    if A <= HOST_MAX_A:
        rows["host"] = host
        hp, hgain, hu, hdc = host()
        # both run the same recurrence: equal gains to rounding (a near tie may go either way)
        assert np.max(np.abs(hgain - gain)) <= 1e-7 * float(np.max(gain)), (n, A, q)
    ms = {k: [] for k in rows}
    # the new route and its yardstick back to back, each as often behind the other as in front
    # (a call that follows the host row finds an idle device: about 1 ms at A = 16384); then the
    # other rows, each after a call of its own
    for rep in range(reps):
        for k in ("zdesign", "pivchol", "pivchol", "zdesign"):
            ms[k].append(timed(rows[k]))
    for k in ("ivr", "host"):
        if k in rows:
            rows[k]()
            ms[k] = [timed(rows[k]) for _ in range(max(2, reps // 2))]
    out = {"N": n, "A": A, "q": q, "d": d}
    out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
    out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
    out["zdesign_over_pivchol"] = round(out["zdesign_ms"] / out["pivchol_ms"], 3)
    for k in ("ivr", "host"):
        if k in rows:
            out[k + "_over_zdesign"] = round(out[k + "_ms"] / out["zdesign_ms"], 2)
        else:
            out[k] = "does not fit"
    out["var_left"] = round(float((zvar0 - gain.sum()) / zvar0), 4)
    npad = (n + 63) // 64 * 64
    try:
        split = kernel_split(e.timeline(zdesign), Ap, npad, q)
        out["zdesign_kernels_ms"] = {k: round(v, 4) for k, v in split.items()}
        split = pivchol_split(e.timeline(pivchol), Ap, q)
        out["pivchol_kernels_ms"] = {k: round(v, 4) for k, v in split.items()}
    except Exception as err:  # the profiler's table is finite: the timings above stand without it
        out["zdesign_kernels_ms"] = "unavailable: %s" % err
    return out


def integral_rows(e, fit, h, w, n, d, s, reps=7):
    """A refit, a single-vector solve and ``integral`` (state there; another measure each time)."""
    mu, cov = measure(d)
    rs = np.random.RandomState(5)
    rhs = rs.randn(n)
    keys = iter(range(1, 10 ** 6))

    def fresh():
        return fit.integral(mu + 1e-3 * next(keys), cov)

    rows = {"refit": lambda: fit.refit(h, w, s), "solve": lambda: fit.solve(rhs),
            "integral_warm": lambda: fit.integral(mu, cov), "integral_new_measure": fresh,
            "integral_weights_warm": lambda: fit.integral(mu, cov, want_weights=True)}
    fit.integral(mu, cov), fit.solve(rhs), fresh()
    ms = {k: [] for k in rows}
    for _ in range(reps):
        for k in ("solve", "integral_warm", "integral_new_measure", "integral_weights_warm"):
            ms[k].append(timed(rows[k]))
    for _ in range(3):
        ms["refit"].append(timed(rows["refit"]))
        fit.solve(rhs)  # (the block inverses back, as the other rows found them)
    out = {"N": n, "d": d}
    out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
    out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
    return out


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [4096, 16384]
    d, s = 3, 0.1
    e = Engine(0)
    for n in sizes:
        rs = np.random.RandomState(n)
        x = np.asfortranarray(rs.uniform(-5, 5, size=(d, n)))
        y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
        h, w = 1.1, np.full(d, 2.0)
        fit = e.gp_fit(x, y, h, w, s)
        try:
            print(json.dumps(integral_rows(e, fit, h, w, n, d, s)), flush=True)
            shapes = [(A, 64) for A in (4096, 16384, 65536)]
            if n == 4096:
                shapes += [(16384, 1), (16384, 256)]
            for A, q in shapes:
                reps = 6 if A <= 16384 and n <= 4096 else 3
                print(json.dumps(run(e, fit, x, h, w, n, A, q, d, s, reps)), flush=True)
        finally:
            fit.close()
    e.close()


if __name__ == "__main__":
    main()
