"""sdc_set_plan_forecast / sdc_get_plan_forecast / sdc_forecast_traces on the CPU side: declared in the header, exported and bound with
the ABI still at 313; sdc_plan_forecast's ctypes mirror has the C compiler's size, offsets and member order; a null handle is refused
before anything else; sdc_forecast.hip cross-compiles for gfx950 with no scratch and no spills, the code object's metadata gives neither
kernel a private segment, and the occupancy the compiler reports is the recorded one; the Python argument rules (dc_rl_amd/_args.py) and
the agents' `forecast` argument, which need no GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from dc_rl_amd import _args as A
from dc_rl_amd import _lib as L
from tests.plan_util import assert_c_layout, assert_no_scratch_or_spills, entry_point_header, kernel_resources

KERNELS = {"sdc_forecast_fill_kernel", "sdc_forecast_swap_kernel"}
# wavefronts per SIMD the compiler reports (18 and 24 VGPRs, no LDS: the most a SIMD holds)
OCCUPANCY = {"sdc_forecast_fill_kernel": 8, "sdc_forecast_swap_kernel": 8}


def test_entry_points_are_declared_exported_and_bound_at_abi_313():
    hdr = entry_point_header("sdc_set_plan_forecast", ["h", "fc"], "sdc_forecast.hip")
    entry_point_header("sdc_get_plan_forecast", ["h", "out"], "sdc_forecast.hip")
    entry_point_header("sdc_forecast_traces", ["h", "n_entries", "truth", "out", "stream"], "sdc_forecast.hip")
    assert re.search(r"\bint sdc_set_plan_forecast\(sdc_handle\* h, const sdc_plan_forecast\* fc\);", hdr)
    assert re.search(r"\bint sdc_get_plan_forecast\(const sdc_handle\* h, sdc_plan_forecast\* out\);", hdr)
    for name, value in (("PERFECT", 0), ("PERSISTENCE", 1), ("DAILY", 2), ("VALUES", 3)):
        m = re.search(r"#define SDC_FORECAST_%s (\d+)" % name, hdr)
        assert m and int(m.group(1)) == value == getattr(L, "FORECAST_" + name) == L.FORECAST_MODES[name.lower()], name
    assert not re.search(r"SDC_DEBUG_\w*FORECAST", hdr)      # (no debug flag came with it)
    assert L.FORECAST_CHANNELS == ("workload", "carbon", "temperature", "wet_bulb")


def test_forecast_mirror_has_the_c_layout(tmp_path):
    assert_c_layout(tmp_path, "sdc_plan_forecast", L.SdcPlanForecast, ["mode", "values_entries", "values"])
    assert L.SdcPlanForecast.mode.size == 16 and L.SdcPlanForecast.values.size == C.sizeof(C.c_void_p)


def test_null_handle_is_refused():
    lib = L.load()
    f = L.SdcPlanForecast()
    assert lib.sdc_set_plan_forecast(None, C.byref(f)) == -2
    assert b"sdc_set_plan_forecast: null handle" in lib.sdc_last_error()
    assert lib.sdc_get_plan_forecast(None, C.byref(f)) == -2
    assert b"sdc_get_plan_forecast: null handle" in lib.sdc_last_error()
    assert lib.sdc_forecast_traces(None, 3, 0, None, None) == -2
    assert b"sdc_forecast_traces: null handle" in lib.sdc_last_error()


def test_forecast_kernels_compile_for_gfx950_without_scratch_or_spills_at_the_recorded_occupancy():
    per = kernel_resources("sdc_forecast.hip")
    assert_no_scratch_or_spills(per, KERNELS)
    assert {k: u["Occupancy"] for k, u in per.items()} == OCCUPANCY, per
    assert all(u["LDS Size"] == 0 for u in per.values()), per


def test_code_object_shows_no_private_segment(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in L.HIPCC_FLAGS if f != "-shared"]
    obj = str(tmp_path / "sdc_forecast.co")
    subprocess.run([hipcc] + flags + ["-c", "--cuda-device-only", "--no-gpu-bundle-output", "sdc_forecast.hip", "-o", obj], cwd=L.CSRC,
                   check=True, capture_output=True, timeout=600)
    readelf = os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "llvm-readelf")
    notes = subprocess.run([readelf, "--notes", obj], check=True, capture_output=True, text=True).stdout
    private = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", notes)]
    symbols = set(re.findall(r"\.symbol:\s*(\S+)\.kd", notes))
    assert symbols == KERNELS and private == [0, 0], (symbols, private)
    assert all(int(x) == 0 for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", notes))


def test_forecast_argument_rules():
    assert A.forecast_modes("w") == [0, 0, 0, 0]
    assert A.forecast_modes("w", workload="persistence", carbon=2, temperature=None, wet_bulb="values") == [1, 2, 0, 3]
    assert A.forecast_modes("w", carbon=7) == [0, 7, 0, 0]      # (a code out of range is the library's to refuse)
    assert A.forecast_mode_names([1, 2, 0, 3]) == dict(workload="persistence", carbon="daily", temperature="perfect", wet_bulb="values")
    with pytest.raises(ValueError, match="w: carbon = 'tomorrow' is not a forecast mode"):
        A.forecast_modes("w", carbon="tomorrow")
    with pytest.raises(ValueError, match="w: wet_bulb must be a forecast mode's name"):
        A.forecast_modes("w", wet_bulb=1.5)
    with pytest.raises(ValueError, match="'humidity' is not a forecast channel"):
        A.forecast_modes("w", humidity="daily")
    A.forecast_entries("w", 1, 0)
    A.forecast_entries("w", L.MARK_MAX_STEPS + 2, 1000)
    for n, left in ((0, 10), (L.MARK_MAX_STEPS + 3, 1000)):
        with pytest.raises(ValueError, match="outside"):
            A.forecast_entries("w", n, left)
    with pytest.raises(ValueError, match="past the end of an episode"):
        A.forecast_entries("w", 6, 3)


class _Env:
    """what an agent's first decision asks of an env before it plans, on the CPU"""

    def __init__(self):
        import torch
        self.n_envs, self.device, self.config, self.set = 2, torch.device("cpu"), dict(auto_reset=True, episode_steps=12), []

    def steps_to_episode_end(self):
        return 12

    def set_plan_forecast(self, **kw):
        self.set.append(kw)

    def sync_groups(self, R):
        pass

    def plan(self, *a, **kw):
        raise StopIteration

    plan_cem = plan_cem_groups = plan


def test_agents_set_their_forecast_on_the_env_before_the_first_decision():
    from dc_rl_amd.agents import CEMMPCAgent, GroupCEMMPCAgent, ShootingMPCAgent
    every = dict(workload="daily", carbon="daily", temperature="daily", wet_bulb="daily")
    for make in (lambda **kw: ShootingMPCAgent(2, 3, **kw), lambda **kw: CEMMPCAgent(2, 1, 1, 3, **kw),
                 lambda **kw: GroupCEMMPCAgent(2, 1, 1, 3, **kw)):
        for forecast, want in ((None, []), ("daily", [every]), (dict(carbon="persistence"), [dict(carbon="persistence")])):
            env, agent = _Env(), make(forecast=forecast)
            for _ in range(2):      # (set once, not at every decision)
                with pytest.raises(StopIteration):
                    agent.act(env)
            assert env.set == want, (forecast, env.set)
