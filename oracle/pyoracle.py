"""ctypes binding of the CPU oracle (oracle/libsdc_oracle.so).

TEST INFRASTRUCTURE ONLY: importable from tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg.  The product package (dc_rl_amd/) must never import this module.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsdc_oracle.so")

MAX_RACKS = 64
HIST_CAP = 10000
QUEUE_CAP = 1000
OBS_DIM = 53
INFO_DIM = 40

INFO_COLS = [
    "ls_original_workload", "ls_shifted_workload", "ls_tasks_in_queue", "ls_norm_tasks_in_queue",
    "ls_tasks_dropped", "ls_tasks_processed", "ls_oldest_task_age", "ls_average_task_age",
    "ls_overdue_penalty", "ls_computed_tasks", "ls_current_hour",
    "ls_hist0", "ls_hist1", "ls_hist2", "ls_hist3", "ls_hist4",
    "dc_ITE_total_power_kW", "dc_CT_total_power_kW", "dc_Compressor_total_power_kW",
    "dc_HVAC_total_power_kW", "dc_total_power_kW", "dc_crac_setpoint_delta", "dc_crac_setpoint",
    "dc_cpu_workload_fraction", "dc_int_temperature", "dc_exterior_ambient_temp", "dc_water_usage",
    "bat_action", "bat_SOC", "bat_CO2_footprint", "bat_avg_CI",
    "bat_total_energy_without_battery_KWh", "bat_total_energy_with_battery_KWh",
    "norm_CI", "outside_temp", "day", "hour", "fault", "reserved0", "reserved1",
]
INFO_IDX = {k: i for i, k in enumerate(INFO_COLS)}


class Params(C.Structure):
    _fields_ = [
        ("R", C.c_int),
        ("rack_n", C.c_double * MAX_RACKS), ("rack_full", C.c_double * MAX_RACKS),
        ("rack_idle", C.c_double * MAX_RACKS), ("rack_supply", C.c_double * MAX_RACKS),
        ("rack_return", C.c_double * MAX_RACKS),
        ("m_cpu", C.c_double), ("c_cpu", C.c_double), ("rs_cpu", C.c_double),
        ("m_fan", C.c_double), ("c_fan", C.c_double), ("rs_fan", C.c_double),
        ("itfan_ref_p", C.c_double), ("itfan_ref_v_ratio", C.c_double), ("it_fan_full_load_v", C.c_double),
        ("c_air", C.c_double), ("rho_air", C.c_double), ("crac_supply_pu", C.c_double),
        ("ct_fan_ref_p", C.c_double), ("ctafr", C.c_double),
        ("min_temp", C.c_double), ("max_temp", C.c_double),
        ("bat_capacity", C.c_double),
        ("queue_max_len", C.c_int),
        ("reward_method", C.c_int * 3),
    ]


class Env(C.Structure):
    _fields_ = [
        ("W", C.POINTER(C.c_double)), ("C", C.POINTER(C.c_double)), ("NC", C.POINTER(C.c_double)),
        ("T", C.POINTER(C.c_double)), ("WB", C.POINTER(C.c_double)), ("NT", C.POINTER(C.c_double)),
        ("win_lo", C.c_int), ("win_len", C.c_int),
        ("cursor", C.c_int), ("day", C.c_int), ("hour", C.c_double), ("t_end", C.c_int),
        ("q_day", C.c_int * QUEUE_CAP), ("q_hour", C.c_double * QUEUE_CAP),
        ("q_head", C.c_int), ("q_len", C.c_int),
        ("ls_norm_tasks_in_queue", C.c_double), ("ls_oldest_age", C.c_double), ("ls_avg_age", C.c_double),
        ("ls_hist", C.c_double * 5),
        ("stpt", C.c_double), ("has_last_delta", C.c_int), ("last_delta", C.c_int),
        ("consecutive", C.c_int), ("scale", C.c_int),
        ("bat_load", C.c_double),
        ("hist", C.c_double * HIST_CAP), ("hist_len", C.c_int), ("hist_pos", C.c_int),
        ("scratch", C.c_double * (2 * HIST_CAP)),
    ]


_lib = None


def build(force: bool = False) -> str:
    src = os.path.join(HERE, "sdc_oracle.c")
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(
            os.path.getmtime(src), os.path.getmtime(os.path.join(HERE, "sdc_oracle.h"))):
        subprocess.check_call(["make", "-C", HERE, "-s"] + (["-B"] if force else []))
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        dp = C.POINTER(C.c_double)
        L.sdco_env_init.argtypes = [C.POINTER(Env)]
        L.sdco_episode_begin.argtypes = [C.POINTER(Env), C.POINTER(Params), dp, dp, dp, dp, dp, dp, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.sdco_step.argtypes = [C.POINTER(Env), C.POINTER(Params), C.POINTER(C.c_int32), C.POINTER(C.c_float), dp, dp]
        L.sdco_step.restype = C.c_int
        L.sdco_normalize_energy.argtypes = [dp, C.c_int, C.c_double]
        L.sdco_normalize_energy.restype = C.c_double
        L.sdco_percentile_linear.argtypes = [dp, C.c_int, C.c_double]
        L.sdco_percentile_linear.restype = C.c_double
        L.sdco_hour_sincos.argtypes = [C.c_double, dp, dp]
        L.sdco_polyfit_slope.argtypes = [dp, C.c_int]
        L.sdco_polyfit_slope.restype = C.c_double
        L.sdco_extract_features.argtypes = [dp, C.c_int, C.c_double, dp]
        L.sdco_dc_model.argtypes = [C.POINTER(Params), C.c_double, C.c_double, C.c_double, C.c_double, dp,
                                    C.POINTER(C.c_uint)]
        L.sdco_chiller_power.argtypes = [C.c_double, C.c_double, C.c_double]
        L.sdco_chiller_power.restype = C.c_double
        L.sdco_battery_step.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, dp]
        L.sdco_battery_step.restype = C.c_uint
        L.sdco_size_datacenter.argtypes = [C.POINTER(Params), C.c_double, dp]
        L.sdco_run_steps.argtypes = [C.POINTER(Env), C.POINTER(Params), C.POINTER(C.c_int32), C.c_long, C.c_int,
                                     C.c_int, C.c_int, dp]
        L.sdco_run_steps.restype = C.c_long
        _lib = L
    return _lib


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def make_params(rack_n, rack_full, rack_idle, rack_supply, rack_return, scal: dict) -> Params:
    p = Params()
    R = len(rack_n)
    p.R = R
    for name, arr in (("rack_n", rack_n), ("rack_full", rack_full), ("rack_idle", rack_idle),
                      ("rack_supply", rack_supply), ("rack_return", rack_return)):
        dst = getattr(p, name)
        for i in range(R):
            dst[i] = float(arr[i])
    for k in ("m_cpu", "c_cpu", "rs_cpu", "m_fan", "c_fan", "rs_fan", "itfan_ref_p", "itfan_ref_v_ratio",
              "it_fan_full_load_v", "c_air", "rho_air", "crac_supply_pu", "ct_fan_ref_p", "ctafr", "min_temp",
              "max_temp", "bat_capacity"):
        setattr(p, k, float(scal[k]))
    p.queue_max_len = int(scal.get("queue_max_len", 1000))
    for i, m in enumerate(scal.get("reward_method", (0, 0, 0))):
        p.reward_method[i] = int(m)
    return p


def params_from_fixture(d) -> Params:
    scal = {k[len("static_"):]: d[k] for k in d.files if k.startswith("static_") and d[k].ndim == 0}
    if "meta_reward_method" in d.files:
        scal["reward_method"] = [int(m) for m in d["meta_reward_method"]]
    return make_params(d["static_rack_n"], d["static_rack_full"], d["static_rack_idle"], d["static_rack_supply"],
                       d["static_rack_return"], scal)


class OracleEnv:
    """One scalar env; keeps the numpy windows alive for the C side."""

    def __init__(self, params: Params):
        self.L = lib()
        self.p = params
        self.e = Env()
        self.L.sdco_env_init(C.byref(self.e))
        self._keep = None

    def begin(self, W, Cc, NC, T, WB, NT, win_lo, init_day, init_hour, steps):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (W, Cc, NC, T, WB, NT)]
        self._keep = arrs
        obs = np.zeros(OBS_DIM, dtype=np.float32)
        self.L.sdco_episode_begin(C.byref(self.e), C.byref(self.p), *[_dptr(a) for a in arrs], int(win_lo),
                                  int(len(arrs[0])), int(init_day), int(init_hour), int(steps),
                                  obs.ctypes.data_as(C.POINTER(C.c_float)))
        return obs

    def step(self, act):
        a = np.ascontiguousarray(act, dtype=np.int32)
        obs = np.zeros(OBS_DIM, dtype=np.float32)
        rew = np.zeros(3, dtype=np.float64)
        info = np.zeros(INFO_DIM, dtype=np.float64)
        done = self.L.sdco_step(C.byref(self.e), C.byref(self.p), a.ctypes.data_as(C.POINTER(C.c_int32)),
                                obs.ctypes.data_as(C.POINTER(C.c_float)), _dptr(rew), _dptr(info))
        return obs, rew, int(done), info
