"""sdc_clone_envs on the CPU side: declared, exported and bound at ABI 313; its translation unit cross-compiles for gfx950 with no
scratch memory (a bandwidth kernel: scratch would add a private-memory round trip per lane)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from dc_rl_amd import _lib as L

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_clone_is_declared_exported_and_bound_at_abi_313():
    hdr = open(os.path.join(ROOT, "include", "sustaindc_hip.h")).read()
    assert re.search(r"#define SDC_ABI_VERSION 313\b", hdr)
    decl = re.search(r"int sdc_clone_envs\(([^)]*)\);", hdr)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == \
        ["h", "src", "dst", "n", "obs", "share_obs", "stream"], decl
    assert L.ABI_VERSION == 313 and "sdc_clone_envs" in L.EXPORTS and "sdc_clone.hip" in L.SOURCES
    L.build()
    lib = C.CDLL(L.LIB_PATH)
    assert lib.sdc_version() == 313
    assert hasattr(lib, "sdc_clone_envs")


def test_clone_kernel_compiles_for_gfx950_without_scratch():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    flags = [f for f in L.HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc] + flags + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "sdc_clone.hip",
                            "-o", os.path.join(td, "o.o")], cwd=L.CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Function Name: sdc_clone_kernel" in r.stderr
    u = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m:
            u[m.group(1).strip()] = int(m.group(2))
    assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert u["Occupancy"] >= 4, u
