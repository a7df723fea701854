"""Time of one slab step (slab_step_kernel, csrc/slab.h) against its workgroup count, in its
512-thread and its 256-thread form -- the table behind launch_slab_step's rule
(csrc/k_panel.hip, BQ_SLAB8_ROUNDS).  Every step of a sweep is bracketed by HIP events
(Engine.timeline); a step of T tile rows has T (T + 1) / 2 workgroups per matrix.

    python tools/slab_step_time.py            # one matrix (N = 5120: the tail of 4736 rows) and
                                              # stacked batches 5 x 1024, 16 x 768
    python tools/slab_step_time.py 1:3008 5:1024
"""
import contextlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_quadrature_amd import Engine  # noqa: E402

REPS = 7


@contextlib.contextmanager
def engine_env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(0, probes=True)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        yield eng
    finally:
        eng.close()


def spd(n, seed):
    rs = np.random.RandomState(seed)
    A = rs.rand(n, n)
    return np.asfortranarray(A + A.T + n * np.eye(n))


def steps(rows, batch):
    """{workgroups: [us, ...]} of the slab steps among timeline rows: the step's work is
    (m^2 64 + m 64^2) batch with m = 64 T rows below the panel."""
    out = {}
    for cls, _, t0, t1, work in rows:
        if cls != "syrk_trailing_small":
            continue
        # m (m + 64) = work / (64 batch)
        m = 0.5 * (-64.0 + np.sqrt(64.0 * 64.0 + 4.0 * work / (64.0 * batch)))
        T = int(round(m / 64.0))
        out.setdefault(T * (T + 1) // 2 * batch, []).append(1e3 * (t1 - t0))
    return out


def measure(eng, batch, n):
    acc = {}
    if batch == 1 and n >= 3072:
        A = spd(n, n)
        dA, dinfo = eng.alloc(8 * n * n), eng.alloc(64)
        for rep in range(REPS + 1):
            eng.upload(dA, A)
            rows = eng.timeline(lambda: eng._check(
                eng._lib.bq_potrf_dev(eng._ctx, dA, n, n, dinfo)))
            if rep:
                for k, v in steps(rows, 1).items():
                    acc.setdefault(k, []).extend(v)
        eng.free(dA), eng.free(dinfo)
        return acc
    src = np.concatenate([spd(n, n + b).T.ravel() for b in range(batch)])
    for rep in range(REPS + 1):
        buf = src.copy()
        route = []
        rows = eng.timeline(lambda: route.append(eng.probe_potrf_batch(buf, batch, n, None, n, n * n)))
        assert route[0][1][0] == "slab", route
        if rep:
            for k, v in steps(rows, batch).items():
                acc.setdefault(k, []).extend(v)
    return acc


def main():
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or \
        [(1, 5120), (5, 1024), (16, 768)]
    forms = (("512 thr", {"BQ_SLAB8_ROUNDS": "1000000"}), ("256 thr", {"BQ_POTF2_8W": "0"}))
    res = {}
    for name, env in forms:
        with engine_env(env) as eng:
            for case in cases:
                res[(name, case)] = measure(eng, *case)
    for case in cases:
        print("batch %d, N = %d: us per step, median of %d (min)" % (case + (REPS,)))
        print("%8s %6s | %16s %16s | %s" % ("wgs", "/256", forms[0][0], forms[1][0], "512 - 256"))
        a, b = res[(forms[0][0], case)], res[(forms[1][0], case)]
        for k in sorted(set(a) & set(b)):
            if k < 36:
                continue
            ma, mb = float(np.median(a[k])), float(np.median(b[k]))
            print("%8d %6.2f | %8.2f (%5.2f) %8.2f (%5.2f) | %+6.2f"
                  % (k, k / 256.0, ma, min(a[k]), mb, min(b[k]), ma - mb), flush=True)


if __name__ == "__main__":
    main()
