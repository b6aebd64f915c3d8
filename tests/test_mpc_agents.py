"""CEMMPCAgent.rollout_stats and GroupCEMMPCAgent.rollout_stats on the CPU, against the engine stub that records what the agents ask of
it (tests/plan_util.AgentStub): what the closed-loop call is handed on a fresh agent, after an act() one step earlier and after the
episode step went backwards, and what the agent carries afterwards.  N = 6 envs, R = 3 (G = 2 groups), H = 4; the expected values are
written out from the two methods as they stood before they became one."""
import pytest
import torch

from dc_rl_amd.agents import CEMMPCAgent, GroupCEMMPCAgent
from tests.plan_util import AgentStub

N, R, H = 6, 3, 4
KW = dict(n_elite=2, n_iters=3, horizon=H, seed=9, alpha=0.25, p_min=0.01)
# (the agent, the carried arrays' leading dimension, what the closed-loop call gets beside the shared arguments)
CASES = [pytest.param(lambda: CEMMPCAgent(5, **KW), N, dict(M=5), id="per-env"),
         pytest.param(lambda: GroupCEMMPCAgent(R, **KW), N // R, dict(R=R), id="groups")]
SHARED = dict(H=H, n_iters=3, E=2, warm_start=True, seed=9, alpha=0.25, p_min=0.01, idle_action=(1, 1, 2), reward_weights=(1.0, 1.0, 1.0),
              gamma=1.0, info_weights=None)


def _handed(env, lead, own, **want):
    """the last closed-loop call got the shared arguments, the class's `own` and `want`, and arrays of the carried layout; a `sync`
    argument exactly when `want` names one"""
    c = dict(env.loops[-1])
    probs, best_seq = c.pop("probs"), c.pop("best_seq")
    assert c == dict(SHARED, **own, **want), c
    assert probs.shape == (H, lead, 3, 3) and probs.dtype == torch.float64
    assert best_seq.shape == (H, lead, 3) and best_seq.dtype == torch.int32
    return probs, best_seq


def _carried(ag, lead, call, steps):
    """the agent carries the first `steps` steps of what call number `call` left in the arrays"""
    assert ag._probs.dtype == torch.float64 and torch.equal(ag._probs, torch.full((steps, lead, 3, 3), float(call), dtype=torch.float64))
    assert ag._best_seq.dtype == torch.int32 and torch.equal(ag._best_seq, torch.full((steps, lead, 3), call, dtype=torch.int32))


@pytest.mark.parametrize("make, lead, own", CASES)
def test_the_first_call_of_a_fresh_agent(make, lead, own):
    grouped = "R" in own
    env, ag = AgentStub(n_envs=N, episode_steps=12), make()
    env.carry = (4, 3)
    res = ag.rollout_stats(env, 3)
    # nothing to resume; the group agent syncs as its first act() would, the per-env agent is given no `sync` argument at all
    _handed(env, lead, own, n_steps=3, resume_steps=0, draw=0, into=None, **(dict(sync=True) if grouped else {}))
    assert "sync" in env.loops[-1] if grouped else "sync" not in env.loops[-1]
    assert res.mpc.steps == 4 and env.syncs == [] and env.calls == []
    assert (ag.draw, ag.last, ag.last_horizon, ag._step, getattr(ag, "syncs", None)) == (3, None, 4, 2, 1 if grouped else None)
    _carried(ag, lead, 1, 4)


@pytest.mark.parametrize("make, lead, own", CASES)
def test_calls_after_an_act_and_after_the_episode_step_went_backwards_and_refused_ones(make, lead, own):
    grouped = "R" in own
    sync = lambda due: dict(sync=due) if grouped else {}
    env, ag = AgentStub(n_envs=N, episode_steps=12), make()
    env.t = 8      # 4 steps left: act() plans 3
    ag.act(env)
    assert (ag.draw, ag.last_horizon, ag._step, getattr(ag, "syncs", None)) == (1, 3, 8, 1 if grouped else None)
    assert env.syncs == ([(0, R)] if grouped else [])
    # one step later, with warm start: the carried length is resumed, the carried tensors are the arrays' first rows, no sync
    env.step()
    env.carry = (2, 2)
    first = object()
    ag.rollout_stats(env, 2, into=first)
    probs, best_seq = _handed(env, lead, own, n_steps=2, resume_steps=3, draw=1, into=first, **sync(False))
    k, a, j = torch.arange(3).view(3, 1, 1, 1), torch.arange(3).view(1, 1, 3, 1), torch.arange(3).view(1, 1, 1, 3)
    assert torch.equal(probs[:3], (1 + k / 16.0 + (3 * a + j) / 256.0).expand(3, lead, 3, 3).to(torch.float64))      # decision 1's
    assert torch.equal(best_seq[:3], (100 + 10 * k[..., 0] + a[..., 0]).expand(3, lead, 3).to(torch.int32))
    assert (ag.draw, ag.last, ag.last_horizon, ag._step, getattr(ag, "syncs", None)) == (3, None, 2, 10, 1 if grouped else None)
    _carried(ag, lead, 1, 2)
    # the episode step went backwards: the group agent syncs and drops the carry, the per-env agent resumes nothing
    assert env.t == 11
    env.t = 0
    env.carry = (4, 5)
    ag.rollout_stats(env, 5)
    _handed(env, lead, own, n_steps=5, resume_steps=0, draw=3, into=None, **sync(True))
    assert (ag.draw, ag.last, ag.last_horizon, ag._step, getattr(ag, "syncs", None)) == (8, None, 4, 4, 2 if grouped else None)
    _carried(ag, lead, 2, 4)
    # refused calls -- one that would have resumed, one that would have synced -- leave draw, syncs and the carry as they were
    env.refuse = True
    for t, resume, due in ((5, 4, False), (0, 0, True)):
        env.t = t
        before = (ag._probs, ag._best_seq)
        with pytest.raises(ValueError, match="refused"):
            ag.rollout_stats(env, 1)
        _handed(env, lead, own, n_steps=1, resume_steps=resume, draw=8, into=None, **sync(due))
        assert (ag.draw, ag.last_horizon, ag._step, getattr(ag, "syncs", None)) == (8, 4, 4, 2 if grouped else None)
        assert ag._probs is before[0] and ag._best_seq is before[1] and env.t == t
        _carried(ag, lead, 2, 4)
    # a call whose last decision idled carries nothing on
    env.refuse, env.t, env.carry = False, 5, (0, 1)
    ag.rollout_stats(env, 1)
    _handed(env, lead, own, n_steps=1, resume_steps=4, draw=8, into=None, **sync(False))
    assert (ag.draw, ag.last, ag.last_horizon, ag._step, getattr(ag, "syncs", None)) == (9, None, 0, 5, 2 if grouped else None)
    assert ag._probs is None and ag._best_seq is None
    assert env.syncs == ([(0, R)] if grouped else [])      # (the closed-loop calls sync inside the library, not through sync_groups)


def test_both_classes_document_their_own_call():
    assert "rollout_cem_stats" in CEMMPCAgent.rollout_stats.__doc__ and "rollout_cem_groups_stats" not in CEMMPCAgent.rollout_stats.__doc__
    assert "rollout_cem_groups_stats" in GroupCEMMPCAgent.rollout_stats.__doc__ and "syncs" in GroupCEMMPCAgent.rollout_stats.__doc__
