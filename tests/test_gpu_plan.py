"""Planning on the device (SdcEngine.plan / SustainDCVecEnv.plan / ShootingMPCAgent over sdc_plan) held to `lookahead` and to the
call's stated arithmetic restated in torch fp64 from a twin engine's rollouts.

 1. plan with the default objective equals lookahead (returns, score, every state field, the engine's output tensors) at 130 and
    4 096 envs;  2. a discounted, weighted objective with info columns, bit for bit;  3. the selection rule;  4. the chunked output
    block (debug_flags PLAN_DEBUG_TWO_STEPS) against the unchunked one;  5. the large-batch rollout path (12 288 envs);  6. the refusals, each of
    which leaves the engine untouched;  7. the vector env with an agent subset;  8. the shooting MPC agent.

NOT in verify mode (debug_flags DEBUG_VERIFY), although the project's parity tests usually are: sdc_rollout refuses verify mode ("verify mode
checks single steps"), so neither `lookahead` nor `rollout` -- the references here -- nor sdc_plan, which takes sdc_rollout's path, run
in it; test 6 checks that refusal.  The rings hold 128 keys and the episodes 96 steps, as in tests/test_gpu_mark.py."""
import ctypes as C

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import ShootingMPCAgent, SustainDCVecEnv
from dc_rl_amd.engine import PlanResult
from tests.plan_util import RSV, _outputs, _twins, objective, planner_refusals, refusal_engines, refused
from tests.test_gpu_clone import _acts
from tests.test_gpu_mark import _assert_rewound, _grab, _mk, _same_out, _same_state

pytestmark = pytest.mark.gpu


def _cands(M, K, N, g):
    import torch
    return torch.randint(0, 3, (M, K, N, 3), dtype=torch.int32, generator=g).cuda()


def _pz(x):
    """-0.0 -> +0.0, every other value as it is: the int64 view then compares values"""
    import torch
    return (x + 0.0).contiguous().view(torch.int64)


def _objective(rew, info, w, gamma, cols):
    """sdc_plan's arithmetic (include/sustaindc_hip.h) from one candidate's rew [K, N, 3] / info [K, N, 44]: element-wise fp64
    multiplies and adds in the stated order -> (returns [N, 3], score [N])"""
    import torch
    K, N = rew.shape[0], rew.shape[1]
    returns = torch.zeros((N, 3), dtype=torch.float64, device=rew.device)
    score = torch.zeros((N,), dtype=torch.float64, device=rew.device)
    gk = 1.0
    for k in range(K):
        if k:
            gk = gk * gamma
        r = rew[k].double()
        returns = returns + r * gk
        s = (r[:, 0] * w[0] + r[:, 1] * w[1]) + r[:, 2] * w[2]
        for key, cw in cols.items():
            s = s + info[k][:, L.INFO_IDX[key]].double() * cw
        score = score + s * gk
    return returns, score


@pytest.mark.parametrize("N", [130, 4096])
def test_plan_with_the_default_objective_equals_lookahead(N):
    import torch
    (a, b), g = _twins(N)
    M, K = 3, 5
    cand = _cands(M, K, N, g)
    kernel = b.last_step_kernel()
    kept, before = _outputs(b), _grab(b)
    ref = a.lookahead(cand)
    res = b.plan(cand)
    assert isinstance(res, PlanResult)
    assert res.returns.shape == (M, N, 3) and res.returns.dtype == torch.float64 and res.returns.is_cuda
    assert res.score.shape == (M, N) and res.best.shape == (N,) and res.action.shape == (N, 3)
    assert res.best.dtype == torch.int32 and res.action.dtype == torch.int32
    assert torch.equal(res.returns, ref), (res.returns != ref).nonzero()[:4].tolist()
    assert not torch.equal(ref[0], ref[1])
    # score with weights 1, 1, 1 and gamma 1 against the returns (fp32 rewards of a few steps: every fp64 addition is exact)
    R = res.returns
    assert torch.equal(res.score, (R[..., 0] + R[..., 1]) + R[..., 2])
    # B's state: what it was before the call to the bit (the stamps cleared), and A's -- every field bit for bit but the ones that
    # depend on which re-centring request found which slot inside a launch, which two engines on one trajectory share by the project's
    # rule for them (tests/test_gpu_mark.py _same_state)
    _assert_rewound(b, before, "after the plan")
    _same_state(a, b, "plan against lookahead")
    for nm, x in kept.items():
        assert torch.equal(getattr(b, nm).view(torch.uint8), x.view(torch.uint8)), nm
    x = _acts(N, g)
    a.step(x)
    b.step(x)
    _same_out(a, b, "the step after")
    assert b.last_step_kernel() == kernel == a.last_step_kernel()
    if N == 4096:
        assert kernel == "sdc_dynamics_fast_kernel"
    a.close()
    b.close()


def test_discounted_weighted_objective_with_info_columns_bit_for_bit():
    import torch
    N, M, K = 130, 2, 7
    (b, twin), g = _twins(N)
    cand = _cands(M, K, N, g)
    w, gamma = (0.5, 2.0, -1.0), 0.9
    three = {L.INFO_COLS[0]: 0.25, "bat_CO2_footprint": -1e-3, L.INFO_COLS[-1]: 3.0}
    eight = dict(three, dc_water_usage=-0.5, ls_tasks_dropped=-2.0, dc_total_power_kW=1e-4, bat_SOC=1.5, energy_z=-0.75)
    assert len(eight) == L.PLAN_MAX_COLS and RSV not in [L.INFO_IDX[k] for k in eight]
    # the twin takes the same launches: mark, then per candidate a rollout and a rewind
    mk = twin.mark(max_steps=K)
    outs = []
    for c in range(M):
        o = twin.rollout(cand[c])
        outs.append((o[2].clone(), o[4].clone()))
        twin.rewind(mk)
    for cols in (three, eight):
        res = b.plan(cand, reward_weights=w, gamma=gamma, info_weights=cols)
        for c in range(M):
            returns, score = _objective(outs[c][0], outs[c][1], w, gamma, cols)
            assert torch.equal(_pz(res.returns[c]), _pz(returns)), (len(cols), c, "returns")
            assert torch.equal(_pz(res.score[c]), _pz(score)), (len(cols), c, "score", (res.score[c] - score).abs().max().item())
    # the columns matter, and so does the discount
    plain = b.plan(cand, reward_weights=w, gamma=gamma)
    assert not torch.equal(plain.score, res.score) and torch.equal(plain.returns, res.returns)
    assert not torch.equal(b.plan(cand, reward_weights=w).score, plain.score)
    b.close()
    twin.close()


def test_selection_takes_the_lowest_candidate_with_the_highest_score():
    import torch
    N, K = 130, 4
    (b,), g = _twins(N, n=1)
    ar = torch.arange(N, device=b.device)
    cand = _cands(5, K, N, g)
    res = b.plan(cand)
    top = res.score.max(0).values
    unique = (res.score == top).sum(0) == 1
    assert bool(unique.any()) and len(torch.unique(res.best)) > 1
    assert torch.equal(res.best[unique].long(), res.score.argmax(0)[unique])
    assert torch.equal(res.score[res.best.long(), ar], top)
    assert torch.equal(res.action, cand[res.best.long(), 0, ar])
    # ties: candidates 1 and 3 repeat candidate 0
    tie = cand[:4].clone()
    tie[1] = tie[0]
    tie[3] = tie[0]
    res = b.plan(tie)
    assert torch.equal(res.score[1], res.score[0]) and torch.equal(res.score[3], res.score[0])
    assert not bool(((res.best == 1) | (res.best == 3)).any())
    two_wins = res.score[2] > res.score[0]
    assert bool(two_wins.any()) and not bool(two_wins.all())
    assert torch.equal(res.best, torch.where(two_wins, 2, 0).to(torch.int32))
    assert torch.equal(res.action, tie[res.best.long(), 0, ar])
    # one candidate
    res = b.plan(cand[:1])
    assert not bool(res.best.any()) and torch.equal(res.action, cand[0, 0])
    b.close()


def test_chunked_output_block_gives_the_unchunked_results():
    import torch
    N, M, K = 130, 3, 5
    whole = _twins(N, n=1)[0][0]
    (chunked,), g = _twins(N, n=1, debug_flags=L.PLAN_DEBUG_TWO_STEPS)      # (chunks of 2 + 2 + 1 steps)
    cand = _cands(M, K, N, g)
    kw = dict(reward_weights=(1.0, 0.5, 2.0), gamma=0.95, info_weights={"bat_CO2_footprint": -1e-3, L.INFO_COLS[-1]: 1.0})
    ra, rb = whole.plan(cand, **kw), chunked.plan(cand, **kw)
    for nm in ("returns", "score", "best", "action"):
        assert torch.equal(getattr(ra, nm), getattr(rb, nm)), nm
    assert len(torch.unique(ra.best)) > 1
    assert whole.steps_to_episode_end() == chunked.steps_to_episode_end()
    for t in range(10):
        x = _acts(N, g)
        oa, ob = whole.step(x), chunked.step(x)
        for nm, u, v in zip(("obs", "share_obs", "rew", "done"), oa, ob):
            assert torch.equal(u, v), (t, nm)
        u, v = oa[4].clone(), ob[4].clone()
        u[:, RSV] = 0
        v[:, RSV] = 0
        assert torch.equal(u, v), (t, "info")
    whole.close()
    chunked.close()


def test_large_batch_rollout_path_equals_lookahead():
    import torch
    N, M, K = 12288, 2, 3      # csrc/sdc_dispatch.hpp SDC_WIDE_ROLLOUT_MIN_ENVS: a rollout is K launches of the lane-per-env kernel
    (a, b), g = _twins(N, history=4)
    assert a.last_step_kernel() == "sdc_dynamics_wide_kernel"
    cand = _cands(M, K, N, g)
    ref = a.lookahead(cand)
    assert a.last_step_kernel() == "sdc_dynamics_wide_kernel"      # (the rollouts' kernel)
    res = b.plan(cand)
    assert b.last_step_kernel() == "sdc_dynamics_wide_kernel"
    assert torch.equal(res.returns, ref)
    R = res.returns
    assert torch.equal(res.score, (R[..., 0] + R[..., 1]) + R[..., 2])
    assert torch.equal(res.action, cand[res.best.long(), 0, torch.arange(N, device=b.device)])
    x = _acts(N, g)
    for nm, u, v in zip(("obs", "share_obs", "rew", "done"), a.step(x), b.step(x)):
        assert torch.equal(u, v), ("the step after", nm)
    a.close()
    b.close()


def test_refusals_leave_the_engine_untouched():
    import torch
    N = 8
    a, fresh, verify, late = refusal_engines(N)
    ones = lambda M, K, n=N: torch.ones((M, K, n, 3), dtype=torch.int32, device=a.device)

    refused(a, "actions must be", lambda: a.plan(ones(2, 3, N + 1)))
    refused(a, "actions must be", lambda: a.plan(ones(2, 3).long()))
    refused(a, "actions must be", lambda: a.plan(ones(2, 3)[0]))
    refused(a, "actions must be", lambda: a.plan(ones(2, 3).cpu()))
    refused(a, "actions must be", lambda: a.plan(ones(0, 3)))
    refused(a, "actions must be", lambda: a.plan(ones(2, 6)[:, ::2]))
    planner_refusals(lambda e, K, **kw: e.plan(ones(2, K), **kw), "MARK_MAX_STEPS", a, fresh, verify, late)
    # what the Python surface cannot send: straight to the library
    x = ones(2, 3)
    out = [torch.empty(2 * N * 3, dtype=torch.float64, device=a.device) for _ in range(2)]
    ints = [torch.empty(N * 3, dtype=torch.int32, device=a.device) for _ in range(2)]
    p = lambda t: C.c_void_p(t.data_ptr())

    def raw(n_cand=2, n_steps=3, obj=None, score=out[1], acts=x):
        rc = a.lib.sdc_plan(a._h, n_cand, n_steps, p(acts) if acts is not None else None, C.byref(obj) if obj is not None else None,
                            p(out[0]), p(score) if score is not None else None, p(ints[0]), p(ints[1]), p(a.obs), p(a.share_obs), a._stream())
        a._refused(rc)

    refused(a, "n_cand", lambda: raw(n_cand=0))
    refused(a, "n_steps", lambda: raw(n_steps=0))
    refused(a, "null array", lambda: raw(score=None))
    refused(a, "null array", lambda: raw(acts=None))
    refused(a, "n_cols", lambda: raw(obj=objective(L.PLAN_MAX_COLS + 1, 0)))
    refused(a, "n_cols", lambda: raw(obj=objective(-1, 0)))
    refused(a, "info column", lambda: raw(obj=objective(1, L.INFO_DIM)))
    refused(a, "info column", lambda: raw(obj=objective(1, -1)))
    # ... and the calls next to them go through: a NULL objective is the default one, the last step of an episode without auto-reset
    raw()
    torch.cuda.synchronize()
    assert torch.equal(out[1][:2 * N].view(2, N), a.plan(x).score)
    assert late.plan(ones(2, 2)).score.shape == (2, N) and late.steps_to_episode_end() == 2
    assert a.plan(ones(2, 37)).returns.shape == (2, N, 3) and a.steps_to_episode_end() == 38
    # a mark taken before a plan is dead after it
    mk = a.mark(max_steps=4)
    a.plan(ones(1, 2))
    refused(a, "dead", lambda: a.rewind(mk))
    for e in (a, fresh, verify, late):
        e.close()


def test_vec_env_plan_with_an_agent_subset():
    import torch
    N, M, K = 16, 3, 4
    args = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True,
            "agents": ["agent_dc", "agent_bat"]}
    a = SustainDCVecEnv(args, n_envs=N, seed=3, months=[6] * N, return_torch=True)
    b = SustainDCVecEnv(args, n_envs=N, seed=3, months=[6] * N, return_torch=True)
    with pytest.raises(ValueError, match="reset"):
        a.plan(torch.ones((M, K, N, 2), dtype=torch.int32))
    a.reset()
    b.reset()
    rng = np.random.default_rng(2)
    for _ in range(5):
        x = torch.as_tensor(rng.integers(0, 3, (N, 2)).astype(np.int32), device=a.engine.device)
        a.step(x)
        b.step(x)
    cand = torch.as_tensor(rng.integers(0, 3, (M, K, N, 2)).astype(np.int32), device=a.engine.device)
    with pytest.raises(ValueError, match="shape"):
        a.plan(cand[:, :, :, :1])
    kw = dict(reward_weights=(0.0, 1.0, 1.0), gamma=0.9, info_weights={"bat_CO2_footprint": -1e-3})
    ra = a.plan(cand, **kw)
    full = torch.ones((M, K, N, 3), dtype=torch.int32, device=a.engine.device)
    full[..., 1:] = cand
    rb = b.engine.plan(full, **kw)
    assert ra.action.shape == (N, 2) and ra.action.dtype == torch.int32
    assert torch.equal(ra.action, rb.action[:, 1:]) and torch.equal(ra.best, rb.best)
    assert torch.equal(ra.score, rb.score) and torch.equal(ra.returns, rb.returns)
    assert torch.equal(ra.action, cand[ra.best.long(), 0, torch.arange(N, device=cand.device)])
    for u, v in zip(a.step(ra.action)[:4], b.step(ra.action)[:4]):
        assert torch.equal(u, v)
    a.close()
    b.close()


def test_shooting_mpc_agent_is_reproducible_and_never_below_do_nothing():
    import torch
    N, M, H, EP_ = 128, 8, 4, 12
    a, b = _mk(N, ep=EP_, seed=8), _mk(N, ep=EP_, seed=8)
    pa, pb = ShootingMPCAgent(M, H, seed=4), ShootingMPCAgent(M, H, seed=4)
    other = ShootingMPCAgent(M, H, seed=5)
    ar = torch.arange(N, device=a.device)
    horizons, differs = [], False
    for t in range(12):
        left = a.steps_to_episode_end()
        xa, xb = pa.act(a), pb.act(b)      # (no call refused: a refusal would raise)
        assert xa.shape == (N, 3) and xa.dtype == torch.int32 and torch.equal(xa, xb), t
        horizons.append(pa.last_horizon)
        assert pa.last_horizon == max(0, min(H, left - 1)) if left >= 2 else pa.last_horizon == 0
        if pa.last is None:
            assert left < 2 and torch.equal(xa, torch.tensor([1, 1, 2], dtype=torch.int32, device=a.device).expand(N, 3))
        else:
            r = pa.last
            assert r.score.shape == (M, N)
            assert bool((r.score[r.best.long(), ar] >= r.score[0]).all()), t
            assert torch.equal(r.score, pb.last.score)
            if t == 0:
                differs = not torch.equal(other.act(a), xa)
        for u, v in zip(a.step(xa), b.step(xb)):
            assert torch.equal(u, v), t
    assert horizons == [4] * 8 + [3, 2, 1, 0], horizons      # the horizon shrinks towards the episode's end; one step left: do nothing
    assert differs
    assert a.steps_to_episode_end() == EP_      # (the 12th step ended the episode: auto-reset)
    a.close()
    b.close()
