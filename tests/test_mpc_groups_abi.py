"""sdc_rollout_cem_groups_stats on the CPU side: declared with its argument names, exported and bound with the ABI still at 313;
sdc_mpc_groups.hip is one of the library's sources; sdc_mpc_group_params has the layout of its ctypes mirror; the library refuses a null
handle before it touches a device; the translation unit cross-compiles for gfx950 with no scratch, no spills and an occupancy of at least
4 for exactly its two kernels, with the figures DESIGN.md section 4.23 states; PlanStats keeps its two-argument form, `diverged` defaults
to None and shows in summary() only when given; GroupCEMMPCAgent.rollout_stats' host logic against a recording stand-in env."""
import re

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests.plan_util import ROOT, assert_c_layout, assert_no_scratch_or_spills, entry_point_header, kernel_resources

ARGS = ["h", "n_steps", "mpc", "objective", "accumulate", "stats", "returns", "counts", "plan_counts", "plan_sums", "diverged", "probs",
        "best_seq", "best_score", "best_action", "step_actions", "cand", "cand_score", "obs", "share_obs", "rew", "done", "info", "final_obs",
        "stream"]


def test_entry_point_is_declared_exported_and_bound_at_abi_313():
    entry_point_header("sdc_rollout_cem_groups_stats", ARGS, "sdc_mpc_groups.hip")
    import dc_rl_amd
    from dc_rl_amd.engine import SdcEngine
    assert callable(SdcEngine.rollout_cem_groups_stats) and callable(dc_rl_amd.GroupCEMMPCAgent.rollout_stats)
    assert dc_rl_amd.GroupCEMMPCAgent.rollout_stats is not dc_rl_amd.CEMMPCAgent.rollout_stats
    assert callable(dc_rl_amd.SustainDCVecEnv.rollout_cem_groups_stats)
    assert not hasattr(dc_rl_amd.SustainDCMultiDeviceVecEnv, "rollout_cem_groups_stats")


def test_mpc_group_params_mirror_has_the_c_layout(tmp_path):
    assert_c_layout(tmp_path, "sdc_mpc_group_params", L.SdcMpcGroupParams,
                    ["horizon", "warm_start", "resume", "resume_steps", "idle_action", "sync_first", "cem"])
    # the embedded struct is sdc_plan_cem_groups' own
    assert dict(L.SdcMpcGroupParams._fields_)["cem"] is L.SdcCemGroupParams


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_rollout_cem_groups_stats(None, 1, None, None, 0, *([None] * 20)) == -2
    assert b"sdc_rollout_cem_groups_stats: null handle" in lib.sdc_last_error()


def test_group_kernels_compile_for_gfx950_without_scratch_or_spills_at_the_figures_design_states():
    per = kernel_resources("sdc_mpc_groups.hip")
    assert_no_scratch_or_spills(per, {"sdc_mpc_group_fold_kernel", "sdc_group_agree_kernel"})
    for k, u in per.items():
        assert u["LDS Size"] == 0, (k, u)      # no LDS, as the kernels' header says
        assert u["Occupancy"] >= 4, (k, u)     # the bar the sibling kernels are held to (tests/test_mpc_stats_abi.py)
    # DESIGN.md section 4.23's table: | `kernel` | VGPRs | LDS | occupancy |
    design = open(f"{ROOT}/DESIGN.md").read()
    sec = design[design.index("### 4.23"):]
    for k, u in per.items():
        row = re.search(r"\| `%s` \| (\d+) \| (\d+) \| (\d+) \|" % k, sec)
        assert row, k
        assert (int(row.group(1)), int(row.group(2)), int(row.group(3))) == (u["VGPRs"], u["LDS Size"], u["Occupancy"]), (k, u, row.group(0))
    # sdc_mpc.hip keeps exactly its two kernels: the start kernel serves the groups as it is
    assert len(re.findall(r"__global__", open(f"{L.CSRC}/sdc_mpc.hip").read())) == 2


def test_plan_stats_diverged_defaults_to_none_and_shows_in_the_summary_only_when_given():
    import torch
    from dc_rl_amd import PlanStats
    from dc_rl_amd.engine import MPCCarry
    counts = torch.zeros((2, 3, 5), dtype=torch.int32)
    counts[:, :, 1] = 4
    sums = torch.tensor([[-2.0, 0.5, 3.0, 1.0], [-1.0, 0.25, 3.0, 1.0]], dtype=torch.float64)
    old = PlanStats(counts, sums)
    assert old.diverged is None
    s = old.summary()
    assert set(s) == {"per_env", "batch", "steps", "planned", "idle"}
    div = torch.tensor([0, 7], dtype=torch.int32)
    for new in (PlanStats(counts, sums, div), PlanStats(counts, sums, diverged=div)):
        assert new.diverged is div
        g = new.summary()
        assert set(g) == set(s) | {"diverged"} and np.array_equal(g["diverged"], [0, 7]) and g["diverged"].dtype == np.int64
        for k in s["per_env"]:
            assert np.array_equal(g["per_env"][k], s["per_env"][k]), k      # the leading dimension reads per group, nothing else changes
    # a leading [E] dimension, as from evaluate
    e = PlanStats(torch.stack([counts, counts]), torch.stack([sums, sums]), torch.stack([div, div])).summary()
    assert e["diverged"].shape == (2, 2)
    # MPCCarry keeps its six-argument form
    c = MPCCarry(None, None, 3, 5, None, None)
    assert c.step_actions is None and (c.steps, c.planned) == (3, 5)
    assert MPCCarry(None, None, 3, 5, None, None, div).step_actions is div


class _Recorder:
    """What GroupCEMMPCAgent.rollout_stats asks of an env: the episode step, and rollout_cem_groups_stats, which records its arguments
    and answers by the library's own schedule (engine.mpc_schedule); `refuse`: the next call raises the engine's ValueError instead"""

    def __init__(self, n_envs=12, episode_steps=20):
        import torch
        self.n_envs, self.device = n_envs, torch.device("cpu")
        self.config = dict(auto_reset=True, episode_steps=episode_steps)
        self.t, self.calls, self.refuse = 0, [], False

    def steps_to_episode_end(self):
        return self.config["episode_steps"] - self.t

    def rollout_cem_groups_stats(self, n_steps, R, H, n_iters, n_elite, *, sync, probs, best_seq, resume_steps, warm_start, draw, **kw):
        from dc_rl_amd.engine import MPCCarry, mpc_schedule
        if self.refuse:
            raise ValueError("sdc_rollout_cem_groups_stats: refused")
        assert probs.shape == (H, self.n_envs // R, 3, 3) and best_seq.shape == (H, self.n_envs // R, 3)
        self.calls.append(dict(n_steps=n_steps, R=R, sync=sync, resume_steps=resume_steps, draw=draw, step=self.t, into=kw.get("into")))
        plan = mpc_schedule(self.steps_to_episode_end(), n_steps, H, True, warm_start, resume_steps)
        self.t = (self.t + n_steps) % self.config["episode_steps"]
        res = type("Res", (), {})()
        res.mpc = MPCCarry(probs, best_seq, plan[-1][0], sum(1 for d in plan if d[1]), None, None, None)
        return res


def test_group_agent_rollout_stats_syncs_as_act_would_and_carries_its_state():
    from dc_rl_amd import GroupCEMMPCAgent
    env = _Recorder()
    ag = GroupCEMMPCAgent(4, n_elite=2, n_iters=2, horizon=3, seed=9)
    first = ag.rollout_stats(env, 5)
    assert env.calls[-1] == dict(n_steps=5, R=4, sync=True, resume_steps=0, draw=0, step=0, into=None)      # the first decision: sync
    assert (ag.syncs, ag.draw, ag._step, ag.last_horizon) == (1, 5, 4, 3) and ag.last is None and ag._probs.shape == (3, 3, 3, 3)
    # a continuation: no sync, the carried result of 3 steps, the draw counter running on
    ag.rollout_stats(env, 4, into=first)
    assert env.calls[-1] == dict(n_steps=4, R=4, sync=False, resume_steps=3, draw=5, step=5, into=first)
    assert (ag.syncs, ag.draw, ag._step) == (1, 9, 8)
    # a refused call leaves the agent as it was
    before = (ag.syncs, ag.draw, ag._step, ag.last_horizon, ag._probs, ag._best_seq)
    env.refuse = True
    with pytest.raises(ValueError, match="refused"):
        ag.rollout_stats(env, 3)
    env.refuse = False
    assert (ag.syncs, ag.draw, ag._step, ag.last_horizon) == before[:4] and ag._probs is before[4] and ag._best_seq is before[5]
    # to the episode's end: 11 steps, the last of them idle -- 10 planned decisions, nothing carried
    ag.rollout_stats(env, 11)
    assert env.calls[-1]["sync"] is False and env.calls[-1]["resume_steps"] == 3
    assert (ag.syncs, ag.draw, ag._step, ag.last_horizon) == (1, 19, 19, 0) and ag._probs is None
    # the episode step has gone backwards: sync again, nothing resumed
    ag.rollout_stats(env, 2)
    assert env.calls[-1] == dict(n_steps=2, R=4, sync=True, resume_steps=0, draw=19, step=0, into=None)
    assert (ag.syncs, ag.draw, ag._step, ag.last_horizon) == (2, 21, 1, 3)
    # without warm start nothing is resumed, and the call still does not sync
    cold = GroupCEMMPCAgent(4, n_elite=2, n_iters=2, horizon=3, seed=9, warm_start=False)
    env2 = _Recorder()
    cold.rollout_stats(env2, 2)
    cold.rollout_stats(env2, 2)
    assert [c["sync"] for c in env2.calls] == [True, False] and [c["resume_steps"] for c in env2.calls] == [0, 0] and cold.draw == 4
