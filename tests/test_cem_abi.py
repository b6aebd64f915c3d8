"""sdc_plan_cem on the CPU side: declared with its argument names, exported and bound with the ABI still at 313; sdc_cem_params' ctypes
mirror has the C compiler's size and offsets; the library refuses a null handle before it touches a device; the translation unit
cross-compiles for gfx950 with no scratch, no spills and an occupancy of at least 4 for exactly its two kernels; CEMMPCAgent's warm
start (the shift of best_seq and probs by a step, the fresh start when the episode step goes backwards) on CPU tensors, against an
engine stub that records what the agent hands to plan_cem."""
import re

from dc_rl_amd import _lib as L
from tests.plan_util import AgentStub as _Stub
from tests.plan_util import assert_c_layout, assert_no_scratch_or_spills, entry_point_header, kernel_resources

ARGS = ["h", "n_steps", "cem", "objective", "probs", "best_seq", "best_score", "best_action", "cand", "cand_score", "obs", "share_obs",
        "stream"]
MEMBERS = ["n_iters", "iter0", "n_cand", "n_elite", "fixed_action", "draw", "seed", "alpha", "p_min"]


def test_cem_entry_point_is_declared_exported_and_bound_at_abi_313():
    hdr = entry_point_header("sdc_plan_cem", ARGS, "sdc_cem.hip")
    m = re.search(r"#define SDC_CEM_MAX_CAND (\d+)", hdr)
    assert m and int(m.group(1)) == L.CEM_MAX_CAND == 64
    import dc_rl_amd
    from dc_rl_amd.agents import CEMMPCAgent
    from dc_rl_amd.engine import CEMResult
    assert dc_rl_amd.CEMMPCAgent is CEMMPCAgent and dc_rl_amd.CEMResult is CEMResult


def test_params_mirror_has_the_c_layout(tmp_path):
    assert_c_layout(tmp_path, "sdc_cem_params", L.SdcCemParams, MEMBERS)
    assert L.SdcCemParams.fixed_action.size == 12 and L.SdcCemParams.seed.size == 8 and L.SdcCemParams.draw.size == 4


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_plan_cem(None, 1, None, None, None, None, None, None, None, None, None, None, None) == -2
    assert b"sdc_plan_cem: null handle" in lib.sdc_last_error()


def test_cem_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_cem.hip")
    assert_no_scratch_or_spills(per, {"sdc_cem_sample_kernel", "sdc_cem_refit_kernel"})
    for k, u in per.items():
        assert u["Occupancy"] >= 4, (k, u)
    # the refit kernel's LDS: four workgroups of four wavefronts fit a CU's 160 KiB, as its header says
    assert 4 * per["sdc_cem_refit_kernel"]["LDS Size"] <= 160 * 1024, per["sdc_cem_refit_kernel"]


def test_warm_start_shifts_by_a_step_and_starts_afresh_when_the_episode_step_goes_backwards():
    import torch
    from dc_rl_amd.agents import CEMMPCAgent
    e = _Stub(n_envs=2, episode_steps=12)
    ag = CEMMPCAgent(n_candidates=6, n_elite=2, n_iters=3, horizon=4, seed=9, alpha=0.25, p_min=0.01)
    third = 1.0 / 3.0
    nothing = torch.tensor([1, 1, 2], dtype=torch.int32)

    def expect_seq(d, K):      # decision d's result moved up by a step: steps 1 .. K-1 of it, then do-nothing
        rows = [[[100 * d + 10 * k + a for a in range(3)]] * 2 for k in range(1, K)] + [[[1, 1, 2]] * 2]
        return torch.tensor(rows, dtype=torch.int32)

    def expect_probs(d, K):
        rows = [[[[d + k / 16.0 + (3 * a + j) / 256.0 for j in range(3)] for a in range(3)]] * 2 for k in range(1, K)]
        rows += [[[[third] * 3] * 3] * 2]
        return torch.tensor(rows, dtype=torch.float64)

    # decision 1: nothing to start from; decisions 2 and 3: the one before, shifted
    a = ag.act(e)
    assert torch.equal(a, torch.tensor([[100, 101, 102]] * 2, dtype=torch.int32))
    c = e.calls[-1]
    assert c["probs"] is None and c["best_seq"] is None and c["draw"] == 0 and c["K"] == 4
    assert (c["n_iters"], c["M"], c["E"], c["seed"], c["alpha"], c["p_min"]) == (3, 6, 2, 9, 0.25, 0.01)
    for d in (1, 2):
        e.step()
        ag.act(e)
        c = e.calls[-1]
        assert c["draw"] == d and c["K"] == 4
        assert c["best_seq"].dtype == torch.int32 and torch.equal(c["best_seq"], expect_seq(d, 4)), d
        assert c["probs"].dtype == torch.float64 and torch.equal(c["probs"], expect_probs(d, 4)), d
    # towards the episode's end the horizon shrinks (11 steps played of 12 at the last planned decision) and the shift follows it
    while e.steps_to_episode_end() > 4:
        e.step()
        ag.act(e)
    assert e.calls[-1]["K"] == 3 and ag.last_horizon == 3
    d = len(e.calls)
    assert torch.equal(e.calls[-1]["best_seq"], expect_seq(d - 1, 3)) and torch.equal(e.calls[-1]["probs"], expect_probs(d - 1, 3))
    e.step()
    ag.act(e)
    assert e.calls[-1]["K"] == 2 and torch.equal(e.calls[-1]["best_seq"], expect_seq(d, 2))
    e.step()
    ag.act(e)
    assert e.calls[-1]["K"] == 1 and torch.equal(e.calls[-1]["best_seq"], nothing.expand(1, 2, 3))
    assert torch.equal(e.calls[-1]["probs"], torch.full((1, 2, 3, 3), third, dtype=torch.float64))
    # one step left: no plan, do nothing
    e.step()
    n = len(e.calls)
    assert e.steps_to_episode_end() == 1
    assert torch.equal(ag.act(e), nothing.expand(2, 3)) and len(e.calls) == n and ag.last is None and ag.last_horizon == 0
    # the episode step goes backwards: both start afresh, and the decision counter goes on
    e.step()
    assert e.steps_to_episode_end() == 12
    ag.act(e)
    c = e.calls[-1]
    assert c["probs"] is None and c["best_seq"] is None and c["draw"] == n and c["K"] == 4
    e.step()
    ag.act(e)
    assert torch.equal(e.calls[-1]["best_seq"], expect_seq(n + 1, 4))
    e.t = 0      # ... also straight from a warm decision
    ag.act(e)
    assert e.calls[-1]["probs"] is None and e.calls[-1]["best_seq"] is None and e.calls[-1]["draw"] == n + 2
    # without warm start every decision starts afresh
    cold = CEMMPCAgent(6, 2, 3, 4, warm_start=False)
    e2 = _Stub()
    for _ in range(3):
        cold.act(e2)
        e2.step()
    assert all(c["probs"] is None and c["best_seq"] is None for c in e2.calls) and [c["draw"] for c in e2.calls] == [0, 1, 2]
