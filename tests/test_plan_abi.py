"""sdc_plan on the CPU side: declared with its argument names, exported and bound with the ABI still at 313; sdc_plan_objective's ctypes
mirror has the C compiler's size and offsets; the library refuses a null handle before it touches a device; the translation unit
cross-compiles for gfx950 with no scratch, no spills and an occupancy of at least 4 for exactly its two kernels."""
import re

from dc_rl_amd import _lib as L
from tests.plan_util import assert_c_layout, assert_no_scratch_or_spills, entry_point_header, kernel_resources

ARGS = ["h", "n_cand", "n_steps", "actions", "objective", "returns", "score", "best", "best_action", "obs", "share_obs", "stream"]
MEMBERS = ["reward_weight", "gamma", "n_cols", "col", "col_weight"]


def test_plan_entry_point_is_declared_exported_and_bound_at_abi_313():
    hdr = entry_point_header("sdc_plan", ARGS, "sdc_plan.hip")
    m = re.search(r"#define SDC_PLAN_MAX_COLS (\d+)", hdr)
    assert m and int(m.group(1)) == L.PLAN_MAX_COLS == 8


def test_objective_mirror_has_the_c_layout(tmp_path):
    assert_c_layout(tmp_path, "sdc_plan_objective", L.SdcPlanObjective, MEMBERS)
    assert L.SdcPlanObjective.col.size == 4 * L.PLAN_MAX_COLS and L.SdcPlanObjective.col_weight.size == 8 * L.PLAN_MAX_COLS


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_plan(None, 1, 1, None, None, None, None, None, None, None, None, None) == -2
    assert b"sdc_plan: null handle" in lib.sdc_last_error()


def test_plan_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_plan.hip")
    assert_no_scratch_or_spills(per, {"sdc_plan_score_kernel", "sdc_plan_select_kernel"})
    for k, u in per.items():
        assert u["Occupancy"] >= 4, (k, u)
