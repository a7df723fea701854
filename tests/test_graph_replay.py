"""Captured launch sequences (csrc/launch_config.h, CapturedSeq): when a plan, a pair's objective
and a fit's vector sweeps capture a hipGraph, replay it, drop it and capture again, told by the
context's counters (Engine.stats: graph_captures / graph_replays / graph_drops) -- bits alone
cannot tell, two routes may agree.  Every result is compared bit for bit with an engine created
with BQ_GRAPH=0 that is taken through the SAME sequence of calls: the same allocation history,
hence the same workspaces on hand and the same routes.

Without a device: the stand-alone check of the type itself (tools/capture_check.hip, on stub
graph calls) and the one list of switches against README's paragraph."""
import contextlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from engine_env import engine_env
from bayesian_quadrature_amd import workloads as wl

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("graph_captures", "graph_replays", "graph_drops")


# ---- without a device ---------------------------------------------------------------------------
def test_capture_check_program(tmp_path):
    """tools/capture_check.hip, built without sanitizers (its header says how to build it with
    them), runs clean: capture, replay, drop on a changed config, every failure path, the
    ineligible contexts, the counters."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "capture_check")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "--offload-arch=gfx950",
                           os.path.join(ROOT, "tools", "capture_check.hip"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout


def _switch_list():
    """[(member, environment name or None)] of BQ_LAUNCH_SWITCHES, read as text."""
    with open(os.path.join(ROOT, "bayesian-quadrature_amd", "csrc", "launch_config.h")) as f:
        text = f.read()
    body = text[text.index("#define BQ_LAUNCH_SWITCHES(X)"):text.index("struct LaunchConfig")]
    found = re.findall(r'^\s*X\((\w+),\s*(?:"(\w+)"|nullptr),', body, re.M)
    return [(m, e or None) for m, e in found]


def test_every_switch_of_the_list_is_in_readme_and_no_other():
    """Every environment name of the one list is in README's switch paragraph, and every BQ_* name
    there is in the list or one of the two that are no context switches."""
    switches = _switch_list()
    envs = {e for _, e in switches if e}
    assert len(switches) == len({m for m, _ in switches}) and len(envs) >= 19, switches
    assert dict(switches)["nb_override"] is None and dict(switches)["use_graph"] == "BQ_GRAPH"
    with open(os.path.join(ROOT, "README.md")) as f:
        paragraphs = f.read().split("\n\n")
    para = [p for p in paragraphs if p.lstrip().startswith("Developer switches")]
    assert len(para) == 1
    named = set(re.findall(r"\bBQ_[A-Z0-9_]+", para[0]))
    assert envs <= named, sorted(envs - named)
    assert named <= envs | {"BQ_FLOW_FAULT", "BQ_GUARD"}, sorted(named - envs)


# ---- on the device ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(engine):
    """(replaying, eager): two new engines, the second with BQ_GRAPH=0."""
    with engine_env({}) as g, engine_env({"BQ_GRAPH": "0"}) as e:
        yield g, e


class Counted(object):
    """The replaying engine's three counters, as steps since the last look."""

    def __init__(self, eng):
        self.eng = eng
        self.last = self.read()

    def read(self):
        s = self.eng.stats()
        return tuple(s[k] for k in COUNTERS)

    def step(self):
        now = self.read()
        d = tuple(a - b for a, b in zip(now, self.last))
        self.last = now
        print("captures %+d replays %+d drops %+d" % d)
        return d


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


@contextlib.contextmanager
def _settings_restored(*engs):
    """The setters' values as engine.config() reads them now, put back on exit."""
    saved = [e.config() for e in engs]

    def restore():
        for e, (nb, la, min_rows) in zip(engs, saved):
            e.set_block(nb)
            e.set_lookahead(la, min_rows)
    try:
        yield restore
    finally:
        restore()


def _plans(engs, B, n, M, c, wscale):
    plans = [e.plan(B, 1, n, M) for e in engs]
    for p in plans:
        p.set_inputs(c["x"], c["y"], c["xo"], c["h"], c["w"] * wscale, c["s"])
    return plans


@gpu
def test_plan_is_captured_once_and_again_after_a_setter(engines):
    """3 x (d = 1, n = 300, M = 40): one capture serves every run until a setter changes the
    configuration; then the graph is dropped and the pass captured again in the same call; a
    setter called with the value in force does neither.  Back under the first settings the
    first bits come back."""
    g, e = engines
    cnt = Counted(g)
    plans = _plans((g, e), 3, 300, 40, wl.c5([0, 1, 2], n=300, m=40), 10)

    def run_results():
        for p in plans:
            p.run()
        res = [p.results() for p in plans]  # (synchronises: no graph is dropped in flight)
        assert _same(*res)
        return res[0]

    with _settings_restored(g, e) as restore:
        try:
            first = run_results()
            run_results()
            assert cnt.step() == (1, 2, 0)
            for eng in (g, e):
                eng.set_block(128)
            run_results()
            assert cnt.step() == (1, 1, 1)
            for eng in (g, e):
                eng.set_block(128)
            run_results()
            assert cnt.step() == (0, 1, 0)
            for eng in (g, e):
                eng.set_lookahead(False)
            run_results()
            assert cnt.step() == (1, 1, 1)
            restore()
            again = run_results()
            assert cnt.step() == (1, 1, 1)
            assert _same(first, again)
        finally:
            for p in plans:
                p.close()


@gpu
def test_one_problem_plan_is_captured_once(engines):
    """(n = 100, M = 20): the first step rides in the assembly launch.  Two runs, one capture."""
    g, e = engines
    cnt = Counted(g)
    c = wl.c2(n=100, m=20)
    c = dict(c, x=c["x"][None], y=c["y"][None], xo=c["xo"][None])
    plans = _plans((g, e), 1, 100, 20, c, 1)
    try:
        for p in plans:
            p.run()
            p.run()
        res = [p.results() for p in plans]
        assert cnt.step() == (1, 2, 0)
        assert _same(*res)
    finally:
        for p in plans:
            p.close()


@gpu
def test_profiled_runs_are_eager_and_replay_resumes_without_a_capture(engines):
    g, e = engines
    cnt = Counted(g)
    plans = _plans((g, e), 3, 300, 40, wl.c5([0, 1, 2], n=300, m=40), 10)
    try:
        for p in plans:
            p.run()
        res = [p.results() for p in plans]
        assert cnt.step() == (1, 1, 0) and _same(*res)
        g.profile(True)
        try:
            plans[0].run()
            under = plans[0].results()
        finally:
            g.profile(False)
        assert cnt.step() == (0, 0, 0) and _same(under, res[1])
        plans[0].run()
        after = plans[0].results()
        assert cnt.step() == (0, 1, 0) and _same(after, res[1])
    finally:
        for p in plans:
            p.close()


@gpu
def test_pair_objective_is_captured_once_and_again_after_a_setter(engines):
    """bq_pair_llh at (ns, nc, S) = (9, 3, 5): two calls with different parameter sets replay one
    capture; set_block drops it."""
    from test_gpu_parity import _pair_problem
    g, e = engines
    cnt = Counted(g)
    ns, nc, S = 9, 3, 5
    xs, ls, xc, dx, rs = _pair_problem(ns, nc, ns + S)
    sets = []
    for _ in range(2):
        sets.append((np.column_stack([rs.uniform(8, 20, S), rs.uniform(1.0, 1.6, S) * dx,
                                      np.full(S, 1e-4)]),
                     np.column_stack([rs.uniform(0.1, 0.4, S), rs.uniform(0.9, 1.3, S) * dx,
                                      np.zeros(S)])))
    pairs = [eng.pair(xs, np.log(ls), ls, xc, None, S) for eng in (g, e)]

    def llh(which):
        res = [p.llh(*sets[which]) for p in pairs]
        assert _same(*res)
        return res[0]

    with _settings_restored(g, e):
        try:
            a, b = llh(0), llh(1)
            assert cnt.step() == (1, 2, 0)
            assert not np.array_equal(a[0], b[0])  # (the second set did arrive)
            for eng in (g, e):
                eng.set_block(64)
            llh(0)
            assert cnt.step() == (1, 1, 1)
        finally:
            for p in pairs:
                p.close()


@gpu
def test_fit_slots_survive_a_refit_and_an_adopted_core_but_not_a_setter(engines):
    """d = 1, n = 250 (npad = 256: the sweeps go through the fit's slots).  A refit keeps the
    pointers and the graphs; an append that grows npad to 320 adopts a new core -- the slots are
    dropped there, which is no configuration change --; set_block costs the slot one recapture."""
    g, e = engines
    cnt = Counted(g)
    c = wl.c2(n=250)
    rs = np.random.RandomState(250)
    b = rs.randn(250)
    fits = [eng.gp_fit(c["x"], c["y"], c["h"], c["w"], c["s"]) for eng in (g, e)]

    def both(fn):
        res = [fn(f) for f in fits]
        assert np.array_equal(res[0], res[1])
        return res[0]

    with _settings_restored(g, e):
        try:
            x1 = both(lambda f: f.solve(b))
            x2 = both(lambda f: f.solve(b))
            both(lambda f: f.alpha())
            assert cnt.step() == (2, 3, 0)   # slots 0 (solve) and 1 (alpha)
            assert np.array_equal(x1, x2)
            for f in fits:
                f.refit(c["h"] * 1.25, c["w"] * 1.5, c["s"])
            x3 = both(lambda f: f.solve(b))
            assert cnt.step() == (0, 1, 0)
            assert not np.array_equal(x1, x3)
            xn = np.linspace(-4.9, 4.9, 10) + 0.37 * (c["x"][1] - c["x"][0])
            for f in fits:
                f.append(xn, wl.norm_logpdf(xn))
            b2 = np.concatenate([b, rs.randn(10)])
            both(lambda f: f.solve(b2))
            assert cnt.step() == (1, 1, 0)
            for eng in (g, e):
                eng.set_block(128)
            both(lambda f: f.solve(b2))
            assert cnt.step() == (1, 1, 1)
        finally:
            for f in fits:
                f.close()


@gpu
def test_eager_engine_never_touches_a_graph(engines):
    """(last in the file: after everything above) BQ_GRAPH=0 leaves all three counters at 0."""
    _, e = engines
    s = e.stats()
    assert [s[k] for k in COUNTERS] == [0, 0, 0], s
