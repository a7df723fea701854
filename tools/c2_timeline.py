"""Where a one-launch slab step's time goes: in-kernel s_memtime stamps of workgroup 0
(the critical path) for every step of a C2 pass (bq_probe_c2_timeline)."""
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from bayesian_quadrature_amd import Engine, _lib as L  # noqa: E402
from bayesian_quadrature_amd import workloads as wl  # noqa: E402

NAMES = ["entry", "frags_loaded", "rows_solved", "tile_loaded", "tile_updated", "potf2_entry",
         "potf2_loaded", "potf2_chain", "potf2_blocks", "potf2_end"]
# The pipelined diagonal tile (BQ_DIAG_PIPE, the default): rows_solved is wave 0 behind B_3, the
# barrier that publishes the last column block; tile_updated is wave 4's lane 0 behind its last
# MFMA; there is no tile_loaded (slot 3 stays 0).  Slots 16-18 / 19-21: wave 4's / wave 0's
# arrivals at B_1 .. B_3.
PIPE_COLS = [0, 1, 2, 4, 5, 6, 7, 8, 9]

if __name__ == "__main__":
    e = Engine(0, probes=True)
    c = wl.c2()
    plan = e.plan(1, 1, 1024, 256)
    plan.set_inputs(c["x"][None], c["y"][None], c["xo"][None], c["h"], c["w"], c["s"])
    for _ in range(5):
        plan.run()
    e.sync()
    nsteps = 16
    st = (C.c_int64 * (160 * nsteps))()
    e._check(e._lib.bq_probe_c2_timeline(e._ctx, plan._h, st, nsteps))
    raw = np.array(list(st), dtype=np.int64).reshape(nsteps, 160)
    pipe = bool((raw[1:15, 16:22] != 0).all())
    cols = PIPE_COLS if pipe else list(range(10))
    names = [NAMES[k] for k in cols]
    t = raw[:, cols]
    d = np.diff(t, axis=1)                       # phase lengths per step
    gap = t[1:, 0] - t[:-1, -1]                  # end of a step's factor -> next step's entry
    out = {"library": L.PROBE_LIB_PATH, "unit": "s_memtime ticks", "diag_pipe": pipe,
           "phases_mean_steps_1_14": {names[i + 1]: float(d[1:15, i].mean())
                                      for i in range(len(cols) - 1)},
           "phases_step_5": {names[i + 1]: int(d[5, i]) for i in range(len(cols) - 1)},
           "step_total_mean": float((t[1:15, -1] - t[1:15, 0]).mean()),
           "solve_end_to_potf2_entry_mean": float((raw[1:15, 5] - raw[1:15, 2]).mean()),
           "gap_end_to_next_entry_mean": float(gap[:14].mean()),
           "gap_all": gap.tolist(),
           "pass_total": int(raw[15, 4] - raw[0, 0])}
    if pipe:
        # wave 0's arrival minus wave 4's at B_1 .. B_3: positive = the update waited for the solve
        lead = raw[1:15, 19:22] - raw[1:15, 16:19]
        out["wave0_minus_wave4_arrival_B1_B3_mean"] = lead.mean(axis=0).tolist()
        out["wave0_minus_wave4_arrival_B1_B3_min"] = lead.min(axis=0).tolist()
        out["solve_intervals_B1_B2_B3_mean"] = [
            float((raw[1:15, 19] - raw[1:15, 1]).mean()),
            float((raw[1:15, 20] - raw[1:15, 19]).mean()),
            float((raw[1:15, 21] - raw[1:15, 20]).mean())]
    # The stores (slots 24 .. 31, slab.h BQ_SSTAMP_STORES).  s_memtime counts per XCD, so workgroups
    # are compared on s_memrealtime (10 ns): workgroup 0's [24] entry / [25] end give its own
    # s_memtime ticks per 10 ns, which places potf2_chain's end ([7]) on that clock; the off-diagonal
    # workgroup's [26] entry / [27] updated / [28] stores acknowledged, and [29 .. 31] the same in its
    # own s_memtime.  Negative offdiag_end_minus_chain_end: the tile was in memory before workgroup 0
    # left its pivot chain.
    if (raw[1:15, 24:29] != 0).all():
        def stores(s):
            f = (raw[s, 9] - raw[s, 0]) / max(1, raw[s, 25] - raw[s, 24])
            chain_end = raw[s, 24] + (raw[s, 7] - raw[s, 0]) / f
            return {"offdiag_entry_minus_wg0_entry_us": 0.01 * float(raw[s, 26] - raw[s, 24]),
                    "offdiag_end_minus_chain_end_us": 0.01 * float(raw[s, 28] - chain_end),
                    "offdiag_entry_to_updated_ticks": int(raw[s, 30] - raw[s, 29]),
                    "offdiag_updated_to_stored_ticks": int(raw[s, 31] - raw[s, 30])}
        out["stores_step_1"] = stores(1)
        per = [stores(s) for s in range(1, 15)]
        out["stores_mean_steps_1_14"] = {k: float(np.mean([p[k] for p in per])) for k in per[0]}
    # The last step (no factor): workgroup 0 from entry to its read-out's stores acknowledged, and
    # the off-diagonal workgroup of the y row's tile row.
    ls = nsteps - 1
    if raw[ls, 25] != 0:
        lcols = [0, 1, 2, 4]
        out["last_step"] = {
            "wg0_phases": {NAMES[b]: int(raw[ls, b] - raw[ls, a]) for a, b in zip(lcols, lcols[1:])},
            "wg0_entry_to_stored_us": 0.01 * float(raw[ls, 25] - raw[ls, 24]),
            "offdiag_entry_to_stored_us": 0.01 * float(raw[ls, 28] - raw[ls, 26]),
            "offdiag_entry_minus_wg0_entry_us": 0.01 * float(raw[ls, 26] - raw[ls, 24]),
            "offdiag_entry_to_updated_ticks": int(raw[ls, 30] - raw[ls, 29]),
            "offdiag_updated_to_stored_ticks": int(raw[ls, 31] - raw[ls, 30])}
    print(json.dumps(out, indent=1))
    plan.close()
    e.close()
