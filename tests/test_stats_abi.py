"""sdc_rollout_stats on the CPU side: declared with its argument names, exported and bound with the ABI still at 313; sdc_stats.hip is one of
the library's sources; the library refuses a null handle before it touches a device; the translation unit cross-compiles for gfx950 with
no scratch, no spills and an occupancy of at least 4 for exactly its two kernels; EpisodeStats.summary() on hand-made CPU tensors against
a NumPy restatement of the reference logger's formulas (harl/envs/sustaindc/sustaindc_logger.py:86-101, :126-149)."""
import re

import numpy as np

from dc_rl_amd import _lib as L
from tests.plan_util import assert_no_scratch_or_spills, entry_point_header, kernel_resources

ARGS = ["h", "n_steps", "actions", "accumulate", "stats", "returns", "counts", "obs", "share_obs", "rew", "done", "info", "final_obs",
        "stream"]


def test_stats_entry_point_is_declared_exported_and_bound_at_abi_313():
    hdr = entry_point_header("sdc_rollout_stats", ARGS, "sdc_stats.hip")
    m = re.search(r"#define SDC_STATS_FIELDS (\d+)", hdr)
    assert m and int(m.group(1)) == L.STATS_FIELDS == 4
    assert re.search(r"enum sdc_stat_field \{ SDC_STAT_SUM = 0, SDC_STAT_MIN, SDC_STAT_MAX, SDC_STAT_NPOS \};", hdr)
    import dc_rl_amd
    from dc_rl_amd.engine import EpisodeStats, SdcEngine
    assert dc_rl_amd.EpisodeStats is EpisodeStats
    assert callable(SdcEngine.rollout_stats) and callable(SdcEngine.evaluate)
    assert callable(dc_rl_amd.SustainDCVecEnv.rollout_stats) and callable(dc_rl_amd.SustainDCVecEnv.evaluate)
    assert not hasattr(dc_rl_amd.SustainDCMultiDeviceVecEnv, "rollout_stats")


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_rollout_stats(None, 1, None, 0, None, None, None, None, None, None, None, None, None, None) == -2
    assert b"sdc_rollout_stats: null handle" in lib.sdc_last_error()


def test_stats_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_stats.hip")
    assert_no_scratch_or_spills(per, {"sdc_stats_reduce_kernel", "sdc_stats_last_kernel"})
    for k, u in per.items():
        assert u["Occupancy"] >= 4, (k, u)
        assert u["LDS Size"] == 0, (k, u)      # no LDS, as the kernels' header says


def _logger(info, steps):
    """The reference logger over one batch: info [K, N, 44] with env n's rows valid for k < steps[n].  per_step (:86-101) adds every env's
    values of a step to ONE set of sums and counts one step per env; episode_log (:130-141) divides by that count.  -> the batch's
    quantities, and the same formulas over each env alone"""
    idx = L.INFO_IDX

    def run(rows):      # rows: the info rows the logger saw
        m = dict(net=0.0, ite=0.0, ct=0.0, chiller=0.0, hvac=0.0, co2=0.0, water=0.0, queue=0.0, dropped=0.0, n=0)
        on = []
        for r in rows:
            m["net"] += r[idx["bat_total_energy_with_battery_KWh"]]
            m["co2"] += r[idx["bat_CO2_footprint"]]
            m["water"] += r[idx["dc_water_usage"]]
            m["queue"] += r[idx["ls_tasks_in_queue"]]
            m["dropped"] += r[idx["ls_tasks_dropped"]]
            m["ite"] += r[idx["dc_ITE_total_power_kW"]]
            m["ct"] += r[idx["dc_CT_total_power_kW"]]
            m["chiller"] += r[idx["dc_Compressor_total_power_kW"]]
            m["hvac"] += r[idx["dc_HVAC_total_power_kW"]]
            if r[idx["dc_HVAC_total_power_kW"]] > 0:
                on.append(r[idx["dc_HVAC_total_power_kW"]])
            m["n"] += 1
        return {"average_net_energy": m["net"] / m["n"], "average_ite_power": m["ite"] / m["n"], "average_ct_power": m["ct"] / m["n"],
                "average_chiller_power": m["chiller"] / m["n"], "average_hvac_power": m["hvac"] / m["n"],
                "average_CO2_footprint": m["co2"] / m["n"], "total_water_usage": m["water"], "total_tasks_in_queue": m["queue"],
                "total_tasks_dropped": m["dropped"], "average_hvac_power_on_use": float(np.mean(on)) if on else float("nan")}

    K, N = info.shape[:2]
    batch = run([info[k, n] for k in range(K) for n in range(N) if k < steps[n]])
    per_env = [run([info[k, n] for k in range(steps[n])]) for n in range(N)]
    return batch, per_env


def test_summary_equals_the_logger_formulas_restated_in_numpy():
    import torch
    from dc_rl_amd.engine import EpisodeStats
    rng = np.random.default_rng(7)
    K, N = 9, 5
    # values with few mantissa bits: every sum below is exact, whatever its order
    info = rng.integers(-8, 64, (K, N, L.INFO_DIM)).astype(np.float64) / 4.0
    hv = L.INFO_IDX["dc_HVAC_total_power_kW"]
    info[:, :, hv] = np.abs(info[:, :, hv])      # a power: never negative ...
    info[::2, 1, hv] = 0.0                       # ... off in some steps of env 1,
    info[:, 3, hv] = 0.0                         # and never on in env 3
    steps = np.array([9, 9, 4, 9, 1])
    live = (np.arange(K)[:, None] < steps[None, :])[:, :, None]
    x = np.where(live, info, 0.0)
    stats = np.stack([x.sum(0), np.where(live, info, np.inf).min(0), np.where(live, info, -np.inf).max(0),
                      (live & (info > 0)).sum(0).astype(np.float64)])
    counts = np.stack([steps, np.zeros(N, dtype=np.int64)], axis=1).astype(np.int32)
    counts[2, 1] = 64
    st = EpisodeStats(torch.from_numpy(stats), torch.zeros((N, 3), dtype=torch.float64), torch.from_numpy(counts))
    assert st.sum.shape == (N, L.INFO_DIM) and torch.equal(st.n_pos, torch.from_numpy(stats[3]))
    assert torch.equal(st.steps, torch.from_numpy(counts[:, 0])) and st.fault.tolist() == [0, 0, 64, 0, 0]
    assert torch.equal(st.col("dc_water_usage"), st.sum[:, L.INFO_IDX["dc_water_usage"]])
    assert torch.equal(st.col("bat_SOC", "max"), st.max[:, L.INFO_IDX["bat_SOC"]])
    for bad in (lambda: st.col("no_such_key"), lambda: st.col("bat_SOC", "mean")):
        try:
            bad()
            raise AssertionError("accepted")
        except ValueError:
            pass
    s = st.summary()
    batch, per_env = _logger(info, steps)
    assert set(s["batch"]) == set(batch) and set(s["per_env"]) == set(batch)
    for name, want in batch.items():
        got = s["batch"][name]
        assert isinstance(got, float) and got == want, (name, got, want)
        for n in range(N):
            g, w = s["per_env"][name][n], per_env[n][name]
            assert (np.isnan(g) and np.isnan(w)) or g == w, (name, n, g, w)
    assert np.isnan(s["per_env"]["average_hvac_power_on_use"][3])
    assert s["steps"].tolist() == steps.tolist() and s["fault"].tolist() == [0, 0, 64, 0, 0]
    # a leading episode dimension (evaluate): every entry is the single episode's
    two = EpisodeStats(torch.from_numpy(np.stack([stats, stats])), torch.zeros((2, N, 3), dtype=torch.float64),
                       torch.from_numpy(np.stack([counts, counts])))
    s2 = two.summary()
    for name in batch:
        assert s2["per_env"][name].shape == (2, N) and s2["batch"][name].shape == (2,)
        assert np.array_equal(s2["per_env"][name][1], s["per_env"][name], equal_nan=True) and s2["batch"][name][0] == s["batch"][name]
