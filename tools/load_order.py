"""Are all of a kernel's first global loads in flight together?  A load that stands behind an
`s_waitcnt vmcnt(..)` is issued only once earlier loads have RETURNED: one more memory round trip
in series, on a path (a one-launch Cholesky step's prologue) that is all latency.  hipcc places
such a wait wherever it schedules the first use of a loaded value, so the source's "every load is
issued here" is a wish until the ISA says so.

    python3 tools/load_order.py [--asm DIR] 'slab_step_kernel<false, 8>' 'panel_step_kernel<8>' ...

For every kernel named (template arguments: bool and int literals) this walks the ISA of
`make asm` (build/asm/k_*.s) from the kernel's entry to its first s_barrier IN TEXT ORDER and
prints the loads, the vmcnt waits and the branches in between, run-length coded, then the number
of vector-memory loads that follow a vmcnt wait (stores are listed too, and a wait that stands
behind one is marked: vmcnt counts stores as well).  Text order, not a walk of the flow graph: a load
counts if ANY wait stands above it, whichever path a wave takes, so 0 means every path is clean.

The text-order walk sees only the prologue that hipcc happens to lay out first (in the pipelined
steps, slab_step_kernel<., 8, true>, the off-diagonal tiles'; the diagonal tiles' two prologues lie
further down).  So the flow graph is walked as well: every path from the kernel's entry to the
first s_barrier ON THAT PATH (or its first store, or its end), both ways at every branch, with
the number of loads pending on the path; a vmcnt(N) wait counts only where more than N are pending (hipcc
puts a vmcnt(0) at the top of a block that has a predecessor with loads in flight, which costs a
wave arriving with nothing pending nothing), and the loads behind such a wait are counted once
each, whichever path finds them.


Exit status 1 if the text-order count is not 0 for any kernel named (or a kernel is not found);
with --paths also if the path count is not 0.  Host-only."""
import argparse
import glob
import os
import re
import sys


def mangled_prefix(spec):
    """'name<false, 8>' -> '_Z16nameILb0ELi8EE' (Itanium ABI, bool / int template arguments)."""
    m = re.match(r"^\s*(\w+)\s*(?:<(.*)>)?\s*$", spec)
    if not m:
        raise SystemExit("cannot parse kernel name %r" % spec)
    name, args = m.group(1), m.group(2)
    out = "_Z%d%s" % (len(name), name)
    if args is None:
        return out
    out += "I"
    for a in args.split(","):
        a = a.strip()
        if a in ("true", "false"):
            out += "Lb%dE" % (a == "true")
        elif re.match(r"^-?\d+$", a):
            out += "Li%sE" % (a if int(a) >= 0 else "n" + a[1:])
        else:
            raise SystemExit("template argument %r of %r is neither bool nor int" % (a, spec))
    return out + "E"


def find_kernel(files, prefix):
    for f in files:
        body, inside = [], False
        for line in open(f):
            if not inside:
                m = re.match(r"^(_Z\w+):", line)
                if m and m.group(1).startswith(prefix):
                    inside = True
                continue
            if line.startswith(".Lfunc_end"):
                return body
            body.append(line)
    return None


LOAD = re.compile(r"^\s+((?:global|flat|buffer|scratch)_load_\w+)")
STORE = re.compile(r"^\s+((?:global|flat|buffer|scratch)_store_\w+)")
WAIT = re.compile(r"^\s+s_waitcnt\b.*\bvmcnt\((\d+)\)")
BRANCH = re.compile(r"^\s+(s_c?branch\w*)\s+(\S+)")
CMP = re.compile(r"^\s+(s_cmpk?_\w+\s+.*)$")


def walk(body):
    """events up to the first s_barrier: (kind, text); and the number of loads behind a wait"""
    ev, waited, behind, last_cmp = [], False, 0, None
    found = stored = False
    for line in body:
        line = line.split(";")[0].rstrip()
        if re.match(r"^\s+s_barrier\b", line):
            found = True
            break
        m = CMP.match(line)
        if m:
            last_cmp = " ".join(m.group(1).split())
        m = LOAD.match(line)
        if m:
            ev.append(("load" + (" BEHIND A WAIT" if waited else ""), m.group(1)))
            behind += waited
            continue
        m = STORE.match(line)
        if m:  # (vmcnt counts stores too: a wait behind one may stand for its acknowledgement)
            ev.append(("store", m.group(1)))
            stored = True
            continue
        m = WAIT.match(line)
        if m:
            ev.append(("wait" + (" behind a store" if stored else ""), "vmcnt(%s)" % m.group(1)))
            waited = True
            continue
        m = BRANCH.match(line)
        if m:
            ev.append(("branch", "%s %s%s" % (m.group(1), m.group(2),
                                               "   (after %s)" % last_cmp if last_cmp else "")))
            last_cmp = None
            continue
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            ev.append(("label", m.group(1)))
    return ev, behind, found


def walk_paths(body):
    """(loads in front of some path's first s_barrier, of them behind a wait that had to wait,
    prologues = distinct first barriers reached)"""
    lines = [l.split(";")[0].rstrip() for l in body]
    label = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            label[m.group(1)] = i
    loads, behind, barriers, seen = set(), set(), set(), set()
    todo = [(0, 0, False)]
    while todo:
        i, pending, waited = todo.pop()
        while i < len(lines):
            if (i, pending, waited) in seen:
                break
            seen.add((i, pending, waited))
            l = lines[i]
            if re.match(r"^\s+s_barrier\b", l):
                barriers.add(i)
                break
            if re.match(r"^\s+s_endpgm\b", l):
                break
            if LOAD.match(l):
                loads.add(i)
                if waited:
                    behind.add(i)
                pending += 1
            elif STORE.match(l):
                break  # (behind a path's first store nothing is a prologue: the read-out's loads)
            else:
                m = WAIT.match(l)
                if m and pending > int(m.group(1)):
                    pending, waited = int(m.group(1)), True
                m = BRANCH.match(l)
                if m and m.group(2) in label:
                    if m.group(1) == "s_branch":
                        i = label[m.group(2)]
                        continue
                    todo.append((label[m.group(2)], pending, waited))
            i += 1
    return len(loads), len(behind), len(barriers)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--asm", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                                  "build", "asm"))
    ap.add_argument("--paths", action="store_true",
                    help="the exit status counts the walk of every path as well")
    ap.add_argument("kernels", nargs="+")
    a = ap.parse_args()
    files = sorted(glob.glob(os.path.join(a.asm, "*-hip-amdgcn-amd-amdhsa-gfx950.s")))
    if not files:
        raise SystemExit("no ISA under %s: run `make -C bayesian-quadrature_amd/csrc asm`" % a.asm)
    bad = 0
    for spec in a.kernels:
        body = find_kernel(files, mangled_prefix(spec))
        print("== %s" % spec)
        if body is None:
            print("   not found (%s...)" % mangled_prefix(spec))
            bad += 1
            continue
        ev, behind, found = walk(body)
        i = 0
        while i < len(ev):  # run-length coded
            j = i
            while j < len(ev) and ev[j][0] == ev[i][0] and (ev[i][0] != "branch" and
                                                            ev[i][0] != "label"):
                j += 1
            j = max(j, i + 1)
            if ev[i][0] in ("branch", "label"):
                print("   %-22s %s" % (ev[i][0], ev[i][1]))
            else:
                texts = [t for _, t in ev[i:j]]
                uniq = []
                for t in texts:
                    if not uniq or uniq[-1][0] != t:
                        uniq.append([t, 0])
                    uniq[-1][1] += 1
                print("   %-22s %s" % (ev[i][0], " ".join("%s%s" % (t, " x%d" % n if n > 1 else "")
                                                          for t, n in uniq)))
            i = j
        if not found:
            print("   (no s_barrier in this kernel: walked to its end)")
        nload = sum(1 for k, _ in ev if k.startswith("load"))
        print("   loads in front of the first s_barrier: %d, of them behind a vmcnt wait: %d"
              % (nload, behind))
        nl, nb, npro = walk_paths(body)
        print("   every path to its first s_barrier or store (%d prologues): %d loads, of them behind a "
              "vmcnt wait that had loads to wait for: %d" % (npro, nl, nb))
        bad += behind != 0 or (a.paths and nb != 0)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
