"""sdc_plan_cem_groups on the CPU side: declared with its argument names, exported and bound with the ABI still at 313;
sdc_cem_group_params' ctypes mirror has the C compiler's size and offsets; the library refuses a null handle before it touches a
device; the translation unit cross-compiles for gfx950 with no scratch and no spills for exactly its two kernels, with the register,
LDS and occupancy figures DESIGN section 4.14 states; GroupCEMMPCAgent's host logic (the warm start's shift by a step, the
re-synchronisation and the fresh start when the episode step goes backwards) on CPU tensors, against an engine stub that records what
the agent asks of it."""
import os
import re

from dc_rl_amd import _lib as L
from tests.plan_util import ROOT, assert_c_layout, assert_no_scratch_or_spills, entry_point_header, kernel_resources
from tests.plan_util import AgentStub as _Stub

ARGS = ["h", "n_steps", "cem", "objective", "probs", "best_seq", "best_score", "best_action", "step_actions", "cand", "cand_score", "obs",
        "share_obs", "stream"]
MEMBERS = ["group_size", "group_base", "n_iters", "iter0", "n_elite", "fixed_action", "draw", "seed", "alpha", "p_min"]
# DESIGN.md section 4.14's table: VGPRs, LDS bytes per workgroup, occupancy in wavefronts per SIMD
FIGURES = {"sdc_cem_group_sample_kernel": (36, 3552, 8), "sdc_cem_group_refit_kernel": (81, 9488, 5)}


def test_entry_point_is_declared_exported_and_bound_at_abi_313():
    hdr = entry_point_header("sdc_plan_cem_groups", ARGS, "sdc_cem_groups.hip")
    m = re.search(r"#define SDC_CEM_MAX_GROUP (\d+)", hdr)
    assert m and int(m.group(1)) == L.CEM_MAX_GROUP == 1024
    import dc_rl_amd
    from dc_rl_amd.agents import GroupCEMMPCAgent
    from dc_rl_amd.engine import GroupCEMResult, SdcEngine
    from dc_rl_amd.vec_env import SustainDCVecEnv
    assert dc_rl_amd.GroupCEMMPCAgent is GroupCEMMPCAgent and dc_rl_amd.GroupCEMResult is GroupCEMResult
    for cls in (SdcEngine, SustainDCVecEnv):
        assert callable(cls.plan_cem_groups) and callable(cls.sync_groups)
    from dc_rl_amd.multi_device import SustainDCMultiDeviceVecEnv
    assert not hasattr(SustainDCMultiDeviceVecEnv, "plan_cem_groups")


def test_params_mirror_has_the_c_layout(tmp_path):
    assert_c_layout(tmp_path, "sdc_cem_group_params", L.SdcCemGroupParams, MEMBERS)
    assert L.SdcCemGroupParams.fixed_action.size == 12 and L.SdcCemGroupParams.seed.size == 8 and L.SdcCemGroupParams.draw.size == 4


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_plan_cem_groups(None, 1, None, None, None, None, None, None, None, None, None, None, None, None) == -2
    assert b"sdc_plan_cem_groups: null handle" in lib.sdc_last_error()


def test_group_kernels_compile_for_gfx950_without_scratch_or_spills_at_the_documented_figures():
    per = kernel_resources("sdc_cem_groups.hip")
    assert_no_scratch_or_spills(per, FIGURES)
    for k, u in per.items():
        assert (u["VGPRs"], u["LDS Size"], u["Occupancy"]) == FIGURES[k], (k, u)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4.14"):]
    for k, (vgprs, lds, occ) in FIGURES.items():
        row = re.search(r"\| `%s` \| (\d+) \| ([\d ]+) \| (\d+) \|" % k, sec)
        assert row, k
        assert (int(row.group(1)), int(row.group(2).replace(" ", "")), int(row.group(3))) == (vgprs, lds, occ), (k, row.group(0))
    # the refit kernel's scores [1024] fp64 are 8 KiB of its LDS; a sample wavefront's LDS leaves the register file as the limit
    assert per["sdc_cem_group_refit_kernel"]["LDS Size"] >= 8 * L.CEM_MAX_GROUP
    assert 32 * per["sdc_cem_group_sample_kernel"]["LDS Size"] <= 160 * 1024


def test_agent_warm_start_shifts_by_a_step_and_resyncs_and_starts_afresh_when_the_episode_step_goes_backwards():
    import pytest
    import torch
    from dc_rl_amd.agents import GroupCEMMPCAgent
    R, G = 3, 2
    e = _Stub(n_envs=R * G, episode_steps=12)
    ag = GroupCEMMPCAgent(R, n_elite=2, n_iters=3, horizon=4, seed=9, alpha=0.25, p_min=0.01)
    third = 1.0 / 3.0
    nothing = torch.tensor([1, 1, 2], dtype=torch.int32)

    def expect_seq(d, K):      # decision d's result moved up by a step: steps 1 .. K-1 of it, then do-nothing; per GROUP
        rows = [[[100 * d + 10 * k + a for a in range(3)]] * G for k in range(1, K)] + [[[1, 1, 2]] * G]
        return torch.tensor(rows, dtype=torch.int32)

    def expect_probs(d, K):
        rows = [[[[d + k / 16.0 + (3 * a + j) / 256.0 for j in range(3)] for a in range(3)]] * G for k in range(1, K)]
        rows += [[[[third] * 3] * 3] * G]
        return torch.tensor(rows, dtype=torch.float64)

    # decision 1: the groups are synchronised first, nothing to start from; the action is every replica's
    a = ag.act(e)
    assert e.syncs == [(0, R)] and ag.syncs == 1
    assert a.shape == (R * G, 3) and torch.equal(a, torch.tensor([[100, 101, 102]] * (R * G), dtype=torch.int32))
    c = e.calls[-1]
    assert c["probs"] is None and c["best_seq"] is None and c["draw"] == 0 and c["K"] == 4 and c["R"] == R
    assert (c["n_iters"], c["E"], c["seed"], c["alpha"], c["p_min"]) == (3, 2, 9, 0.25, 0.01)
    # decisions 2 and 3: the one before, shifted; no further synchronisation inside the episode
    for d in (1, 2):
        e.step()
        ag.act(e)
        c = e.calls[-1]
        assert c["draw"] == d and c["K"] == 4
        assert c["best_seq"].dtype == torch.int32 and torch.equal(c["best_seq"], expect_seq(d, 4)), d
        assert c["probs"].dtype == torch.float64 and torch.equal(c["probs"], expect_probs(d, 4)), d
    assert len(e.syncs) == 1
    # towards the episode's end the horizon shrinks and the shift follows it
    while e.steps_to_episode_end() > 4:
        e.step()
        ag.act(e)
    assert e.calls[-1]["K"] == 3 and ag.last_horizon == 3
    d = len(e.calls)
    assert torch.equal(e.calls[-1]["best_seq"], expect_seq(d - 1, 3)) and torch.equal(e.calls[-1]["probs"], expect_probs(d - 1, 3))
    e.step()
    ag.act(e)
    e.step()
    ag.act(e)
    assert e.calls[-1]["K"] == 1 and torch.equal(e.calls[-1]["best_seq"], nothing.expand(1, G, 3))
    # one step left: no plan, every replica does nothing
    e.step()
    n = len(e.calls)
    assert e.steps_to_episode_end() == 1
    assert torch.equal(ag.act(e), nothing.expand(R * G, 3)) and len(e.calls) == n and ag.last is None and ag.last_horizon == 0
    assert len(e.syncs) == 1
    # the episode step goes backwards: the groups are synchronised again BEFORE the plan, both start afresh, the counter goes on
    e.step()
    assert e.steps_to_episode_end() == 12
    ag.act(e)
    c = e.calls[-1]
    assert e.syncs == [(0, R), (n, R)] and ag.syncs == 2
    assert c["probs"] is None and c["best_seq"] is None and c["draw"] == n and c["K"] == 4
    e.step()
    ag.act(e)
    assert torch.equal(e.calls[-1]["best_seq"], expect_seq(n + 1, 4)) and len(e.syncs) == 2
    e.step()
    ag.act(e)
    e.t = 0      # ... also straight from a warm decision
    ag.act(e)
    assert e.calls[-1]["probs"] is None and e.calls[-1]["best_seq"] is None and len(e.syncs) == 3 and e.syncs[-1] == (len(e.calls) - 1, R)
    with pytest.raises(ValueError, match="group_size"):
        GroupCEMMPCAgent(1)
    with pytest.raises(ValueError, match="n_elite"):
        GroupCEMMPCAgent(4, n_elite=5)
