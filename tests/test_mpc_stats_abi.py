"""sdc_rollout_cem_stats on the CPU side: declared with its argument names, exported and bound with the ABI still at 313; sdc_mpc.hip is one
of the library's sources; the header's #define and enum are the binding's constants; sdc_mpc_params has the layout of its ctypes mirror;
the library refuses a null handle before it touches a device; the translation unit cross-compiles for gfx950 with no scratch, no spills,
no LDS and an occupancy of at least 4 for exactly its two kernels; PlanStats.summary() on hand-made CPU tensors against a NumPy
restatement written out here; EpisodeStats keeps its three-argument form and gains a keyword-only `plan`."""
import re

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests.plan_util import assert_c_layout, assert_no_scratch_or_spills, entry_point_header, kernel_resources

ARGS = ["h", "n_steps", "mpc", "objective", "accumulate", "stats", "returns", "counts", "plan_counts", "plan_sums", "probs", "best_seq",
        "best_score", "best_action", "cand", "cand_score", "obs", "share_obs", "rew", "done", "info", "final_obs", "stream"]


def test_cem_stats_entry_point_is_declared_exported_and_bound_at_abi_313():
    hdr = entry_point_header("sdc_rollout_cem_stats", ARGS, "sdc_mpc.hip")
    m = re.search(r"#define SDC_PLAN_SUMS (\d+)", hdr)
    assert m and int(m.group(1)) == L.PLAN_SUMS == 4
    assert re.search(r"enum sdc_plan_sum \{ SDC_PLAN_SCORE = 0, SDC_PLAN_GAIN, SDC_PLAN_PLANNED, SDC_PLAN_IDLE \};", hdr)
    assert (L.PLAN_SCORE, L.PLAN_GAIN, L.PLAN_PLANNED, L.PLAN_IDLE) == (0, 1, 2, 3)
    import dc_rl_amd
    from dc_rl_amd.engine import PlanStats, SdcEngine
    assert dc_rl_amd.PlanStats is PlanStats
    assert callable(SdcEngine.rollout_cem_stats) and callable(dc_rl_amd.CEMMPCAgent.rollout_stats)
    for nm in ("rollout_cem_stats", "evaluate"):
        assert callable(getattr(dc_rl_amd.SustainDCVecEnv, nm)), nm
    assert not hasattr(dc_rl_amd.SustainDCMultiDeviceVecEnv, "rollout_cem_stats")


def test_mpc_params_mirror_has_the_c_layout(tmp_path):
    assert_c_layout(tmp_path, "sdc_mpc_params", L.SdcMpcParams,
                    ["horizon", "warm_start", "resume", "resume_steps", "idle_action", "reserved", "cem"])
    # the embedded struct is sdc_plan_cem's own
    assert dict(L.SdcMpcParams._fields_)["cem"] is L.SdcCemParams


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_rollout_cem_stats(None, 1, None, None, 0, *([None] * 18)) == -2
    assert b"sdc_rollout_cem_stats: null handle" in lib.sdc_last_error()


def test_mpc_kernels_compile_for_gfx950_without_scratch_spills_or_lds():
    per = kernel_resources("sdc_mpc.hip")
    assert_no_scratch_or_spills(per, {"sdc_mpc_start_kernel", "sdc_mpc_fold_kernel"})
    for k, u in per.items():
        assert u["LDS Size"] == 0, (k, u)      # no LDS, as the kernels' header says
        assert u["Occupancy"] >= 4, (k, u)     # the bar the sibling reduce kernels are held to (tests/test_stats_abi.py)


def _summary_ref(counts, sums):
    """PlanStats.summary restated: counts [..., N, 3, 5] (n0, n1, n2, switches, last), sums [..., N, 4] (score, gain, planned, idle)"""
    n = counts[..., :3].astype(np.float64)
    steps = n[..., 0] + n[..., 1] + n[..., 2]                       # [..., N, 3]
    sw = counts[..., 3].astype(np.float64)
    trans = np.maximum(steps - 1.0, 1.0)
    env_axis = steps.ndim - 2
    tot = steps.sum(axis=env_axis)                                   # [..., 3]
    safe = np.where(steps > 0, steps, 1.0)
    tsafe = np.where(tot > 0, tot, 1.0)
    score, gain, planned, idle = (sums[..., i] for i in range(4))   # [..., N]
    psafe = np.where(planned > 0, planned, 1.0)
    ptot = planned.sum(axis=-1)
    ptsafe = np.where(ptot > 0, ptot, 1.0)
    per_env = {
        "action_frequency": np.where(steps[..., None] > 0, n / safe[..., None], 0.0),
        "switch_rate": sw / trans,
        "mean_score": np.where(planned > 0, score / psafe, 0.0),
        "mean_gain": np.where(planned > 0, gain / psafe, 0.0),
    }
    batch = {
        "action_frequency": np.where(tot[..., None] > 0, n.sum(axis=env_axis) / tsafe[..., None], 0.0),
        "switch_rate": sw.sum(axis=env_axis) / trans.sum(axis=env_axis),
        "mean_score": np.where(ptot > 0, score.sum(axis=-1) / ptsafe, 0.0),
        "mean_gain": np.where(ptot > 0, gain.sum(axis=-1) / ptsafe, 0.0),
    }
    return per_env, batch, steps.astype(np.int64), planned.astype(np.int64), idle.astype(np.int64)


def _hand_made(rng, N):
    """counts / sums of N envs: env 0 took ONE step, an idle one (no transition, no planned decision: no division by zero), env 1 none at
    all, the others 2 .. 40 steps, the last of them idle, with switches <= steps - 1"""
    counts = np.zeros((N, 3, 5), dtype=np.int32)
    sums = np.zeros((N, 4), dtype=np.float64)
    for e in range(N):
        steps = 1 if e == 0 else (0 if e == 1 else int(rng.integers(2, 41)))
        planned = max(steps - 1, 0)
        sums[e] = [-planned * rng.uniform(0.5, 3.0), planned * rng.uniform(0.0, 0.5), planned, steps - planned]
        for a in range(3):
            split = np.sort(rng.integers(0, steps + 1, size=2))
            counts[e, a, :3] = [split[0], split[1] - split[0], steps - split[1]]
            counts[e, a, 3] = 0 if steps < 2 else int(rng.integers(0, steps))
            counts[e, a, 4] = -1 if steps == 0 else int(rng.integers(0, 3))
    return counts, sums


def _check(got, per_env, batch, steps, planned, idle):
    assert set(got) == {"per_env", "batch", "steps", "planned", "idle"}
    assert set(got["per_env"]) == set(per_env) and set(got["batch"]) == set(batch)
    for k in per_env:
        assert got["per_env"][k].dtype == np.float64 and got["per_env"][k].shape == per_env[k].shape, k
        assert np.array_equal(got["per_env"][k], per_env[k]), k
        assert np.asarray(got["batch"][k]).shape == batch[k].shape, k
        assert np.array_equal(got["batch"][k], batch[k]), k
    assert np.array_equal(got["steps"], steps) and np.array_equal(got["planned"], planned) and np.array_equal(got["idle"], idle)


def test_plan_stats_summary_against_a_numpy_restatement():
    import torch
    from dc_rl_amd import PlanStats
    rng = np.random.default_rng(23)
    N = 6
    counts, sums = _hand_made(rng, N)
    ps = PlanStats(torch.from_numpy(counts), torch.from_numpy(sums))
    # the views
    assert ps.action_counts.shape == (N, 3, 3) and torch.equal(ps.action_counts, ps.counts[:, :, :3])
    assert torch.equal(ps.switches, ps.counts[:, :, 3]) and torch.equal(ps.last_action, ps.counts[:, :, 4])
    for i, nm in enumerate(("score", "gain", "planned", "idle")):
        assert torch.equal(getattr(ps, nm), ps.sums[:, i]), nm
    assert ps.score.data_ptr() == ps.sums.data_ptr()      # views, not copies
    got = ps.summary()
    _check(got, *_summary_ref(counts, sums))
    assert got["per_env"]["action_frequency"].shape == (N, 3, 3) and got["batch"]["switch_rate"].shape == (3,)
    assert got["per_env"]["mean_score"].shape == (N,) and isinstance(got["batch"]["mean_score"], float)
    # the env with one (idle) step: a frequency of 1 on its action, switch rate 0, no planned decision -> mean score 0; the env with no
    # step: zeros; nothing NaN
    assert np.array_equal(got["per_env"]["switch_rate"][0], np.zeros(3)) and np.array_equal(got["per_env"]["action_frequency"][0].sum(-1), np.ones(3))
    assert got["per_env"]["mean_score"][0] == 0.0 and got["per_env"]["mean_gain"][0] == 0.0 and got["idle"][0] == 1
    assert np.array_equal(got["per_env"]["action_frequency"][1], np.zeros((3, 3))) and got["per_env"]["mean_score"][1] == 0.0
    assert all(np.isfinite(v).all() for v in got["per_env"].values()) and all(np.isfinite(v).all() for v in got["batch"].values())
    assert got["per_env"]["mean_score"][2] == sums[2, 0] / sums[2, 2]
    # a leading [E] dimension, as from evaluate
    c2, s2 = _hand_made(rng, N)
    pe = PlanStats(torch.from_numpy(np.stack([counts, c2])), torch.from_numpy(np.stack([sums, s2])))
    got = pe.summary()
    _check(got, *_summary_ref(np.stack([counts, c2]), np.stack([sums, s2])))
    assert got["per_env"]["mean_gain"].shape == (2, N) and got["batch"]["action_frequency"].shape == (2, 3, 3)
    assert got["batch"]["mean_score"].shape == (2,)
    first = ps.summary()
    for k in first["batch"]:
        assert np.array_equal(got["batch"][k][0], first["batch"][k]), k
    # a batch that planned nothing at all
    none = PlanStats(torch.zeros((2, 3, 5), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.float64)).summary()
    assert none["batch"]["mean_score"] == 0.0 and np.array_equal(none["per_env"]["switch_rate"], np.zeros((2, 3)))


def test_episode_stats_keeps_its_three_argument_form_and_takes_a_keyword_only_plan():
    import torch
    from dc_rl_amd import EpisodeStats, PlanStats, PolicyStats
    stats, ret, cnt = torch.zeros((4, 2, L.INFO_DIM), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.float64), torch.ones((2, 2), dtype=torch.int32)
    st = EpisodeStats(stats, ret, cnt)
    assert st.plan is None and st.policy is None and st.mpc is None and st.stats is stats
    assert set(st.summary()) == {"per_env", "batch", "steps", "fault"}
    pl = PlanStats(torch.zeros((2, 3, 5), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.float64))
    ps = PolicyStats(torch.zeros((2, 3, 5), dtype=torch.int32), torch.zeros((2, 3, 2), dtype=torch.float64))
    both = EpisodeStats(stats, ret, cnt, ps, plan=pl)
    assert both.plan is pl and both.policy is ps
    with pytest.raises(TypeError):
        EpisodeStats(stats, ret, cnt, ps, pl)      # keyword-only: the positional form stays (stats, returns, counts, policy)


def test_the_host_schedule_of_the_binding_counts_planned_decisions_as_the_agent_would():
    """engine.mpc_schedule, which sizes MPCCarry: 7 steps to the end of a 96-step episode with auto-reset, H = 4"""
    from dc_rl_amd.engine import mpc_schedule
    plan = mpc_schedule(7, 7, 4, True)
    assert [d[0] for d in plan] == [4, 4, 4, 3, 2, 1, 0]
    assert [d[1] for d in plan] == [True] * 6 + [False]
    assert [d[2] for d in plan] == [True] + [False] * 5 + [False]
    assert [d[3] for d in plan[:6]] == list(range(6))
    assert [d[2] for d in mpc_schedule(7, 3, 4, True, warm_start=False)] == [True] * 3
    assert [d[2] for d in mpc_schedule(20, 2, 4, True, resume_steps=3)] == [True, False]      # K = 4 exceeds the 3 carried steps
    assert [d[2] for d in mpc_schedule(20, 2, 4, True, resume_steps=4)] == [False, False]
    assert [d[0] for d in mpc_schedule(3, 3, 4, False)] == [3, 2, 0]      # without auto-reset the last step may be planned for
