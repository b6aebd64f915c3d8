"""sdc_mark_row_bytes / sdc_mark_envs / sdc_rewind_envs on the CPU side: declared, exported and bound with the ABI still at 313; a mark
row is roundup256(1964 + 12 K) bytes and below 1/40 of a 672-step snapshot row for every K <= 64; the library refuses a null handle
before it touches a device; the translation unit cross-compiles for gfx950 with no scratch, no spills and an occupancy of at least 4
for exactly its two kernels."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from dc_rl_amd import _lib as L

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ARGS = {
    "sdc_mark_row_bytes": ["max_steps"],
    "sdc_mark_envs": ["h", "envs", "n", "max_steps", "rows", "manifest", "obs", "share_obs", "stream"],
    "sdc_rewind_envs": ["h", "envs", "n", "rows", "manifest", "obs", "share_obs", "stream"],
}
SNAPSHOT_ROW_672 = 145920      # a snapshot row at 672-step episodes


def _roundup256(x):
    return (x + 255) // 256 * 256


def test_mark_entry_points_are_declared_exported_and_bound_at_abi_313():
    hdr = open(os.path.join(ROOT, "include", "sustaindc_hip.h")).read()
    assert re.search(r"#define SDC_ABI_VERSION 313\b", hdr)
    m = re.search(r"#define SDC_MARK_MANIFEST (\d+)", hdr)
    assert m and int(m.group(1)) == L.MARK_MANIFEST
    m = re.search(r"#define SDC_MARK_MAX_STEPS (\d+)", hdr)
    assert m and int(m.group(1)) == L.MARK_MAX_STEPS
    enum = re.search(r"enum sdc_mark_manifest \{(.*?)\};", hdr, re.S)
    assert enum and len(re.findall(r"\bSDC_MARK_M_\w+", enum.group(1))) == L.MARK_MANIFEST
    for name, args in ARGS.items():
        decl = re.search(r"\b%s\(([^)]*)\);" % name, hdr)
        assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == args, (name, decl)
        assert name in L.EXPORTS
    assert L.ABI_VERSION == 313 and "sdc_mark.hip" in L.SOURCES
    L.build()
    lib = C.CDLL(L.LIB_PATH)
    assert lib.sdc_version() == 313
    for name in ARGS:
        assert hasattr(lib, name), name


def test_row_bytes_formula_and_size_against_a_snapshot_row():
    lib = L.load()
    for k in (1, 16, 64, L.MARK_MAX_STEPS):
        assert lib.sdc_mark_row_bytes(k) == _roundup256(1964 + 12 * k), k
    assert lib.sdc_mark_row_bytes(16) == 2304 and lib.sdc_mark_row_bytes(64) == 2816
    for k in (0, -1, L.MARK_MAX_STEPS + 1, 1 << 30):
        assert lib.sdc_mark_row_bytes(k) == 0, k
    for k in range(1, 65):
        assert 0 < lib.sdc_mark_row_bytes(k) * 40 < SNAPSHOT_ROW_672, k


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_mark_envs(None, None, 1, 16, None, None, None, None, None) == -2
    assert b"sdc_mark_envs: null handle" in lib.sdc_last_error()
    assert lib.sdc_rewind_envs(None, None, 1, None, None, None, None, None) == -2
    assert b"sdc_rewind_envs: null handle" in lib.sdc_last_error()


def test_mark_kernels_compile_for_gfx950_without_scratch_or_spills():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    flags = [f for f in L.HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc] + flags + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "sdc_mark.hip",
                            "-o", os.path.join(td, "o.o")], cwd=L.CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    per, cur = {}, None
    for line in r.stderr.splitlines():
        f = re.search(r"remark:\s+Function Name: (\S+)", line)
        if f:
            cur = per.setdefault(f.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert set(per) == {"sdc_mark_save_kernel", "sdc_mark_rewind_kernel"}, sorted(per)
    for k, u in per.items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert u["Occupancy"] >= 4, (k, u)
