"""The C-ABI library loads without a GPU and exports every symbol that
include/bqhip.h declares and no hardware probe; the probe library exports those
and every probe of include/bqhip_probe.h; the ctypes tables cover exactly them;
both are linked -Bsymbolic; the product fails loudly (no fallback) when no
device is present."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header="bqhip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bq_[A-Za-z0-9_]+)\s*\(", text)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_symbols_exported():
    from bayesian_quadrature_amd import _lib
    lib = _lib.load_library()
    names = _declared()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), "libbqhip.so does not export %s" % n
    assert not [n for n in _exported(_lib.LIB_PATH) if n.startswith("bq_probe_")]


def test_probe_library_exports_both_headers():
    from bayesian_quadrature_amd import _lib
    lib = _lib.load_probe_library()
    probes = _declared("bqhip_probe.h")
    assert probes and all(n.startswith("bq_probe_") for n in probes)
    for n in _declared() + probes:
        assert hasattr(lib, n), "libbqhip_probe.so does not export %s" % n


def test_ctypes_table_matches_header():
    from bayesian_quadrature_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()
    assert sorted(_lib.PROBE_SIGNATURES) == _declared("bqhip_probe.h")


def test_libraries_bind_their_own_symbols():
    """DT_FLAGS SYMBOLIC (-Wl,-Bsymbolic): calls between a library's own entry points stay inside
    it although both libraries export the bqhip.h names and libbqhip.so is loaded RTLD_GLOBAL."""
    from bayesian_quadrature_amd import _lib
    for path in (_lib.LIB_PATH, _lib.PROBE_LIB_PATH):
        dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True,
                             check=True).stdout
        flags = [ln for ln in dyn.splitlines() if "(FLAGS)" in ln]
        assert flags and "SYMBOLIC" in flags[0].split(), (path, flags)


def test_device_count_and_loud_failure():
    from bayesian_quadrature_amd import _lib, Engine
    n = C.c_int(-1)
    assert _lib.load_library().bq_device_count(C.byref(n)) == 0
    assert n.value >= 0
    if n.value == 0:
        with pytest.raises(RuntimeError):
            Engine(0)


def test_product_does_not_import_oracle():
    # the oracle is test infrastructure: nothing under the product package may
    # mention it
    pkg = os.path.join(ROOT, "bayesian-quadrature_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.lower(), f


def test_null_context_is_rejected():
    from bayesian_quadrature_amd import _lib
    lib = _lib.load_library()
    assert lib.bq_ctx_sync(None) == _lib.BQ_ERR_BAD_ARG
    assert lib.bq_set_block(None, 64) == _lib.BQ_ERR_BAD_ARG


def test_lds_dma_fills_are_waited_for_before_barriers(tmp_path):
    """hipcc orders an LDS-DMA (global_load_lds) only against the issuing wave's own LDS reads: the
    `s_waitcnt vmcnt(0)` the OTHER waves of the workgroup rely on before the barrier is there by
    explicit asm or by luck.  tools/check_ldsdma_waits.py walks the control-flow graph of every
    LDS-DMA kernel in the gfx950 ISA of k_gemm.hip and finds no barrier reachable with a fill in
    flight (round 4: the loop header of trsm_sweep_kernel was one)."""
    import subprocess
    import sys
    src = os.path.join(ROOT, "bayesian-quadrature_amd", "csrc", "k_gemm.hip")
    out = tmp_path / "k_gemm-hip-amdgcn-amd-amdhsa-gfx950.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                           "-fno-fast-math", "--cuda-device-only", "-S", src, "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_ldsdma_waits.py"),
                        str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert "trsm_sweep_kernel" in r.stdout and "gemm_lds_kernel" in r.stdout
