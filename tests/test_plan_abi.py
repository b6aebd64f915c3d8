"""sdc_plan on the CPU side: declared with its argument names, exported and bound with the ABI still at 313; sdc_plan_objective's ctypes
mirror has the C compiler's size and offsets; the library refuses a null handle before it touches a device; the translation unit
cross-compiles for gfx950 with no scratch, no spills and an occupancy of at least 4 for exactly its two kernels."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from dc_rl_amd import _lib as L

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "sustaindc_hip.h")
ARGS = ["h", "n_cand", "n_steps", "actions", "objective", "returns", "score", "best", "best_action", "obs", "share_obs", "stream"]
MEMBERS = ["reward_weight", "gamma", "n_cols", "col", "col_weight"]


def test_plan_entry_point_is_declared_exported_and_bound_at_abi_313():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define SDC_ABI_VERSION 313\b", hdr)
    m = re.search(r"#define SDC_PLAN_MAX_COLS (\d+)", hdr)
    assert m and int(m.group(1)) == L.PLAN_MAX_COLS == 8
    decl = re.search(r"\bint sdc_plan\(([^)]*)\);", hdr)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == ARGS, decl
    assert "sdc_plan" in L.EXPORTS
    assert L.ABI_VERSION == 313 and "sdc_plan.hip" in L.SOURCES
    L.build()
    lib = C.CDLL(L.LIB_PATH)
    assert lib.sdc_version() == 313
    assert hasattr(lib, "sdc_plan")
    assert len(L.load().sdc_plan.argtypes) == len(ARGS)


def test_objective_mirror_has_the_c_layout(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(sdc_plan_objective));']
    src += [f'  printf("{m} %zu\\n", offsetof(sdc_plan_objective, {m}));' for m in MEMBERS]
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-o", exe, str(c)], check=True)
    out = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SdcPlanObjective)
    for m in MEMBERS:
        assert int(out[m]) == getattr(L.SdcPlanObjective, m).offset, m
    assert [f[0] for f in L.SdcPlanObjective._fields_] == MEMBERS
    assert L.SdcPlanObjective.col.size == 4 * L.PLAN_MAX_COLS and L.SdcPlanObjective.col_weight.size == 8 * L.PLAN_MAX_COLS


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_plan(None, 1, 1, None, None, None, None, None, None, None, None, None) == -2
    assert b"sdc_plan: null handle" in lib.sdc_last_error()


def test_plan_kernels_compile_for_gfx950_without_scratch_or_spills():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in L.HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc] + flags + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "sdc_plan.hip",
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
    assert set(per) == {"sdc_plan_score_kernel", "sdc_plan_select_kernel"}, sorted(per)
    for k, u in per.items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert u["Occupancy"] >= 4, (k, u)
