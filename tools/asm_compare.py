"""Did a refactor change the code of a kernel?  Compares the ISA of two `make asm` trees, kernel
by kernel, for the kernels whose names match the patterns given.

    python3 tools/asm_compare.py BEFORE_DIR AFTER_DIR [name-pattern | OLD=>NEW ...]

An argument OLD=>NEW pairs a kernel of BEFORE with the kernel of AFTER whose demangled name is the
BEFORE name with the text OLD replaced by NEW (a template that gained a parameter: 'true>=>true,
false>'); several of them pair it with several kernels.  Without one, names pair with themselves.

Per kernel it prints the code-object metadata of both (VGPRs, spilled VGPRs, spilled SGPRs, LDS
bytes, waves per SIMD), whether the instruction streams are the same text with labels, comments
and symbol names stripped (`same`), and if not, whether the text-order sequence of the "ordered"
instructions -- matrix instructions, global / LDS / scratch loads and stores, s_barrier -- is the
same (`ordered ops same`), with the opcode counts that differ.  Demangled names need c++filt.

Exit status 1 if a kernel's ordered sequence, LDS size, occupancy or spill counts differ, or a
kernel exists on one side only.  Host-only."""
import collections
import glob
import os
import re
import subprocess
import sys

ORDERED = re.compile(r"^(v_mfma_|v_smfma|global_|flat_|buffer_|scratch_|ds_|s_barrier)")


def kernels(asm_dir):
    """{mangled name: (instructions, metadata)} of every kernel under asm_dir"""
    out = {}
    for f in sorted(glob.glob(os.path.join(asm_dir, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        lines = open(f).read().split("\n")
        name, body, info = None, [], {}
        for i, line in enumerate(lines):
            m = re.match(r"^(_Z\w+):", line)
            if m and name is None:
                name, body, info = m.group(1), [], {}
                continue
            if name is None:
                continue
            if line.startswith(".Lfunc_end"):
                for l in lines[i:i + 40]:
                    m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize):? *(\d+)", l)
                    if m:
                        info[m.group(1)] = int(m.group(2))
                out[name] = [body, info]
                name = None
                continue
            l = line.split(";")[0].strip()
            if not l or l.endswith(":") or l.startswith("."):
                continue
            body.append(re.sub(r"\.LBB\w+", "L", re.sub(r"_Z\w+", "SYM", " ".join(l.split()))))
        text = "\n".join(lines)
        for m in re.finditer(r"\.name:\s+(_Z\w+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                             r"\s+\.vgpr_spill_count:\s+(\d+)", text):
            if m.group(1) in out:
                out[m.group(1)][1]["sgpr_spill"] = int(m.group(2))
                out[m.group(1)][1]["vgpr_spill"] = int(m.group(3))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
        return dict(zip(names, (re.sub(r"\(.*$", "", l) for l in r.stdout.split("\n"))))
    except OSError:
        return {n: n for n in names}


def meta(info):
    return "%3d %3d %3d %6d %d" % (info.get("TotalNumVgprs", -1), info.get("vgpr_spill", -1),
                                   info.get("sgpr_spill", -1), info.get("LDSByteSize", -1),
                                   info.get("Occupancy", -1))


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    renames = [a.split("=>") for a in sys.argv[3:] if "=>" in a]
    pats = [re.compile(p) for p in sys.argv[3:] if "=>" not in p] or [re.compile(".")]
    names = sorted(set(before) | set(after))
    pretty = demangle(names)
    by_pretty = {pretty[n]: n for n in after}
    bad = 0
    print("kernel | VGPRs, spilled VGPRs, spilled SGPRs, LDS bytes, waves/SIMD: before -> after | code")
    pairs = []
    for n in names:
        if not any(p.search(pretty[n]) for p in pats):
            continue
        if renames:
            pairs += [(n, by_pretty[pretty[n].replace(a, b)]) for a, b in renames
                      if n in before and a in pretty[n] and pretty[n].replace(a, b) in by_pretty]
            continue
        if n not in before or n not in after:
            print("%s | only %s" % (pretty[n], "before" if n in before else "after"))
            bad += 1
            continue
        pairs.append((n, n))
    for n, n1 in pairs:
        (b0, i0), (b1, i1) = before[n], after[n1]
        op0, op1 = [l.split()[0] for l in b0], [l.split()[0] for l in b1]
        if b0 == b1:
            verdict = "same (%d instructions)" % len(b0)
        else:
            same_ord = [o for o in op0 if ORDERED.match(o)] == [o for o in op1 if ORDERED.match(o)]
            c0, c1 = collections.Counter(op0), collections.Counter(op1)
            d = ", ".join("%s %+d" % (o, c1[o] - c0[o]) for o in sorted(set(c0) | set(c1)) if c0[o] != c1[o])
            verdict = "%s; %d -> %d instructions; counts: %s" % (
                "ordered ops same" if same_ord else "ORDERED OPS DIFFER", len(b0), len(b1), d or "equal")
            bad += not same_ord
        worse = any(i1.get(k, 0) > i0.get(k, 0) for k in ("vgpr_spill", "sgpr_spill")) or any(
            i1.get(k) != i0.get(k) for k in ("LDSByteSize", "Occupancy"))
        bad += worse
        print("%s%s | %s -> %s%s | %s" % (pretty[n], "" if n1 == n else " -> " + pretty[n1], meta(i0),
                                          meta(i1), " WORSE" if worse else "", verdict))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
