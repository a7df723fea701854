"""Joint posterior samples on the device (bq_gp_sample) next to the host route they replace:
python tools/sample_time.py [N ...]

For N in {1024, 4096, 16384} x M in {256, 1024, 4096}, S = 64, d = 3, wall-clock times of the
whole call on a warm fit (block inverses resident, workspaces grown), medians of repeats after a
warm-up, the rows taken in turn within every repeat:
  sample   engine.Fit.sample with the device's normals and a one-entry ladder
  host     what a user did before: predict(want_cov=True), numpy.linalg.cholesky of the M x M
           matrix with the same jitter, numpy normals and the matmul
The jitter is the first entry of the default ladder at which BOTH routes factor (the device finds
its own first; numpy may need the next), so that both do the same work.  And, from the launch
profiler, the kernel time of one sample split into the sweep (cross Gram, forward row sweep, row
reductions), Sigma (Gram of the query points and V V^T), the factorisation and the product (the
normals and tri_sample_kernel).  One JSON line per shape; the host route's factor is checked
against the device's on the way, so that a wrong timing cannot hide a wrong answer."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402

LADDER = (0.0, 1e-12, 1e-10, 1e-8, 1e-6)
S = 64


def stages(tl):
    """Kernel ms of one sample's launches (Engine.timeline rows, in launch order) by stage: the
    second gram-class launch opens Sigma (two launches), the last two are the product."""
    gram = [i for i, r in enumerate(tl) if r[0] == "gram"]
    a, b = gram[1], len(tl) - 2
    ms = [r[3] - r[2] for r in tl]
    return {"sweep": sum(ms[:a]), "sigma": sum(ms[a:a + 2]), "factor": sum(ms[a + 2:b]),
            "product": sum(ms[b:])}


def run(e, n, M, d=3, reps=5):
    rs = np.random.RandomState(n + M)
    x = rs.uniform(-5, 5, size=(d, n))
    y = np.sin(x).sum(axis=0) + 0.1 * rs.randn(n)
    h, w, s = 1.1, np.full(d, 2.0), 0.1
    xo = np.asfortranarray(rs.uniform(-5, 5, size=(d, M)))
    fit = e.gp_fit(x, y, h, w, s)
    try:
        _, _, jitter = fit.sample(xo, S=S, seed=1)  # the device's own first rung
        k0 = h * h / (np.sqrt(2 * np.pi) * w[0]) ** d
        for t in LADDER:
            if t * k0 < jitter * (1 - 1e-12):
                continue
            try:
                _, _, cov = fit.predict(xo, want_mean=False, want_cov=True)
                Lh = np.linalg.cholesky(cov + t * k0 * np.eye(M))
                _, _, jitter, Ld = fit.sample(xo, S=S, seed=1, ladder=(t,), want_chol=True)
                break
            except np.linalg.LinAlgError:
                continue
        else:
            raise RuntimeError("no rung of the ladder factors on both routes")
        # both factor the same matrix: L L^T agree to the rounding of Sigma itself
        scale = k0 + np.max(np.abs(cov))
        assert np.max(np.abs(Lh @ Lh.T - Ld @ Ld.T)) <= 1e-9 * scale, (n, M)

        def sample():
            return fit.sample(xo, S=S, seed=1, ladder=(t,))

        def host():
            mean, _, cov = fit.predict(xo, want_cov=True)
            Lc = np.linalg.cholesky(cov + jitter * np.eye(M))
            return mean[:, None] + Lc @ np.random.standard_normal((M, S))

        rows = {"sample": sample, "host": host}

        def timed(call):
            t0 = time.perf_counter()
            call()
            return (time.perf_counter() - t0) * 1e3

        for call in rows.values():
            timed(call)
        ms = {k: [] for k in rows}
        for _ in range(reps):
            for k, call in rows.items():
                ms[k].append(timed(call))
        out = {"N": n, "M": M, "S": S, "d": d, "jitter_over_k0": t}
        out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
        out.update({k + "_spread_ms": round(float(np.max(v) - np.min(v)), 3) for k, v in ms.items()})
        out["host_over_sample"] = round(out["host_ms"] / out["sample_ms"], 2)
        tl = e.timeline(sample)
        out["sample_kernels_ms"] = {k: round(v, 4) for k, v in stages(tl).items()}
        out["sample_launches"] = len(tl)
        return out
    finally:
        fit.close()


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096, 16384]
    e = Engine(0)
    for n in sizes:
        for M in (256, 1024, 4096):
            print(json.dumps(run(e, n, M, reps=5 if n <= 4096 else 3)), flush=True)
    e.close()


if __name__ == "__main__":
    main()
