"""Planner evaluation over replica groups on the device (SdcEngine.rollout_cem_groups_stats / evaluate(mpc=), GroupCEMMPCAgent.rollout_stats,
SustainDCVecEnv.rollout_cem_groups_stats / evaluate over sdc_rollout_cem_groups_stats) held to the Python loop it replaces.

THE REFERENCE throughout is a twin engine with the same seed, driven by that loop: `a = GroupCEMMPCAgent(...).act(twin)`, then
`twin.rollout_stats(a[None], into=ref)`; its plan arrays are restated in torch in step order, per group, from the agent's
`last.best_score` and the action it played (`_loop`).

THE BAR is every bit: stats, returns, counts; plan_counts and plan_sums; the final probs / best_seq prefix, best_score, best_action and
step_actions; the engines' states and single-step views (tests/test_gpu_mark.py _same_state / _same_out).  info[reserved] is left out
between two engines, as in tests/test_gpu_stats.py.  No case is excluded from any comparison.  `diverged` is all zeros wherever the
groups hold one state, and in case 7 equals, exactly, the count restated on the host from the twin's per-step rew / info / done views.

Shapes (G groups of R replicas): (3, 8) -- 24 envs, 9 lanes of the fold; (5, 6) -- 30 envs, groups that straddle the four-env wavefronts
of the agreement check, whose last wavefront is partial; (2, 64) -- 128 envs, a group over several wavefronts and workgroups.

 1. 10 steps from a reset with sync=True on the three shapes, warm start on and off;  2. the chunked output block (debug_flags bit 14);
 3. continuation: 5 steps, then 5 more with `into=` and `resume_steps`, and `agent.act()` behind `agent.rollout_stats`;  4. the episode's
 end: the horizon shrinks 4, 4, 4, 3, 2, 1, the last step idles (step_actions all idle_action) and auto-resets, the next call syncs
 again, starts fresh, and the replicas equal their leaders again;  5. a persistence forecast, a limit and a terminal term;  6. a fixed
 action, alpha and p_min;  7. the agreement check on a group with a perturbed replica;  8. the refusals, each of which leaves the engine,
 the launch counter and the caller's arrays untouched;  9. through the vector env: evaluate(mpc=), the agent-subset ValueError,
 copy.deepcopy.

96-step episodes, rings of 128 keys, auto-reset on, H = 4, I = 2, E = 2."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import EpisodeStats, GroupCEMMPCAgent, PlanStats, SustainDCVecEnv
from dc_rl_amd.engine import mpc_schedule
from tests.plan_util import refused
from tests.test_gpu_actor_stats import _engine as _actor_engine
from tests.test_gpu_mark import SCHEDULED, _grab, _same_out, _same_state
from tests.test_gpu_stats import _bits

pytestmark = pytest.mark.gpu

EP, H, E, I = 96, 4, 2, 2
RSV = L.INFO_IDX["reserved"]
COLS = [c for c in range(L.INFO_DIM) if c != RSV]
CEM = dict(n_elite=E, n_iters=I, horizon=H, seed=77)
SHAPES = [(3, 8), (5, 6), (2, 64)]
IDLE = [1, 1, 2]


def _engine(N, **kw):
    return _actor_engine(N, actors=None, **kw)


def _agent(R, cls=GroupCEMMPCAgent, **kw):
    return cls(R, **dict(CEM, **kw))


def _fold(counts, sums, played, scores):
    """one decision into the plan arrays, in torch: `played` [G, 3] the action played, `scores` [I, G] of a planned decision or None"""
    import torch
    which = torch.arange(3, dtype=torch.int32, device=played.device)
    last = counts[..., L.POLICY_LAST]
    counts[..., :3] += (played[..., None] == which).to(torch.int32)
    counts[..., L.POLICY_SWITCHES] += ((last >= 0) & (played != last)).to(torch.int32)
    counts[..., L.POLICY_LAST] = played
    if scores is not None:
        sums[:, L.PLAN_SCORE] = sums[:, L.PLAN_SCORE] + scores[-1]
        sums[:, L.PLAN_GAIN] = sums[:, L.PLAN_GAIN] + (scores[-1] - scores[0])
        sums[:, L.PLAN_PLANNED] = sums[:, L.PLAN_PLANNED] + 1.0
    else:
        sums[:, L.PLAN_IDLE] = sums[:, L.PLAN_IDLE] + 1.0


def _plan_arrays(G, dev, plan=None):
    import torch
    if plan is not None:
        return plan[0].clone(), plan[1].clone()
    counts = torch.zeros((G, 3, 5), dtype=torch.int32, device=dev)
    counts[..., L.POLICY_LAST] = -1
    return counts, torch.zeros((G, 4), dtype=torch.float64, device=dev)


def _host_diverged(eng, R):
    """`diverged` of the step the engine's single-step views hold, restated: per group the replicas whose rew, done or info row -- without
    info[reserved] -- differs from their group's first env's in any bit"""
    import torch
    N = eng.n_envs
    lead = torch.arange(N, device=eng.device) // R * R
    info = eng.info.clone()
    info[:, RSV] = 0
    info, rew, done = info.view(torch.int32), eng.rew.contiguous().view(torch.int32), eng.done.to(torch.int32)
    differs = (info != info[lead]).any(1) | (rew != rew[lead]).any(1) | (done != done[lead])
    return differs.view(N // R, R).sum(1).to(torch.int32)


def _loop(twin, agent, n, ref=None, plan=None):
    """n rounds of the loop that exists today on `twin` -> (the EpisodeStats, (plan counts [G, 3, 5], plan sums [G, 4]) restated in step
    order, the last step_actions, the horizons the agent planned over, `diverged` restated per step); `ref` / `plan`: an earlier call's"""
    import torch
    R = agent.group_size
    G = twin.n_envs // R
    counts, sums = _plan_arrays(G, twin.device, plan)
    div = torch.zeros((G,), dtype=torch.int32, device=twin.device)
    a, horizons = None, []
    for _ in range(n):
        a = agent.act(twin)
        horizons.append(agent.last_horizon)
        ref = twin.rollout_stats(a[None], into=ref)
        _fold(counts, sums, a[::R], agent.last.best_score if agent.last is not None else None)
        div += _host_diverged(twin, R)
    return ref, (counts, sums), a.clone(), horizons, div


def _assert_call(got, ref, plan, action, agent, what, diverged=None):
    """a rollout_cem_groups_stats result against the loop's: every bit of the statistics, the plan arrays, the carried prefix, the last
    actions; `diverged`: what the call must have counted (None: zeros)"""
    import torch
    assert isinstance(got, EpisodeStats) and isinstance(got.plan, PlanStats) and got.policy is None
    N, R = ref.counts.shape[0], agent.group_size
    G = N // R
    assert got.plan.counts.shape == (G, 3, L.POLICY_COUNTS) and got.plan.counts.dtype == torch.int32 and got.plan.counts.is_cuda
    assert got.plan.sums.shape == (G, L.PLAN_SUMS) and got.plan.sums.dtype == torch.float64
    assert got.plan.diverged.shape == (G,) and got.plan.diverged.dtype == torch.int32
    assert got.stats.shape == (4, N, L.INFO_DIM) and got.returns.shape == (N, 3) and got.counts.shape == (N, 2)
    assert torch.equal(_bits(got.stats[..., COLS]), _bits(ref.stats[..., COLS])), (what, "stats")
    assert torch.equal(_bits(got.returns), _bits(ref.returns)), (what, "returns")
    assert torch.equal(got.counts, ref.counts), (what, "counts")
    if not torch.equal(got.plan.counts, plan[0]):
        bad = (got.plan.counts != plan[0]).nonzero()
        raise AssertionError((what, "plan_counts", len(bad), bad[:4].tolist()))
    if not torch.equal(_bits(got.plan.sums), _bits(plan[1])):
        bad = (_bits(got.plan.sums) != _bits(plan[1])).nonzero()
        raise AssertionError((what, "plan_sums", len(bad), bad[:4].tolist(), got.plan.sums[:2].tolist(), plan[1][:2].tolist()))
    want = torch.zeros_like(got.plan.diverged) if diverged is None else diverged
    assert torch.equal(got.plan.diverged, want), (what, "diverged", got.plan.diverged.tolist(), want.tolist())
    c = got.mpc
    assert c.steps == agent.last_horizon, (what, c.steps, agent.last_horizon)
    if c.steps:
        assert torch.equal(_bits(c.probs[:c.steps]), _bits(agent._probs)), (what, "probs")
        assert torch.equal(c.best_seq[:c.steps], agent._best_seq), (what, "best_seq")
        assert torch.equal(_bits(c.best_score), _bits(agent.last.best_score)), (what, "best_score")
    assert torch.equal(c.best_action, action[::R]), (what, "best_action")
    assert torch.equal(c.step_actions, action), (what, "step_actions")


def _assert_engines(e, twin, what):
    _same_state(e, twin, what)
    _same_out(e, twin, what)


def _call(e, n, R, agent_kw=None, **kw):
    """rollout_cem_groups_stats on e with the shared CEM parameters"""
    p = dict(CEM, **(agent_kw or {}))
    return e.rollout_cem_groups_stats(n, R, p["horizon"], p["n_iters"], p["n_elite"], seed=p["seed"],
                                      **{k: v for k, v in p.items() if k in ("alpha", "p_min", "warm_start")}, **kw)


@functools.lru_cache(maxsize=None)
def _reference(G, R, warm):
    """the 10-step run from a reset that cases 1 to 3 share at G groups of R: the twin, its agent and the loop's results -- computed
    once, never changed afterwards"""
    twin, agent = _engine(G * R), _agent(R, warm_start=warm)
    return (twin, agent) + _loop(twin, agent, 10)


@pytest.mark.parametrize("G,R", SHAPES)
@pytest.mark.parametrize("warm", [True, False])
def test_ten_steps_from_a_reset_equal_the_python_loop(G, R, warm):
    import torch
    twin, agent, ref, plan, action, horizons, div = _reference(G, R, warm)
    what = f"G = {G}, R = {R}, warm_start = {warm}"
    e = _engine(G * R)
    lead = torch.arange(G * R, device=e.device) // R * R
    assert not torch.equal(e.obs, e.obs[lead])      # the replicas drew resets of their own: the sync is the call's
    got = _call(e, 10, R, dict(warm_start=warm), sync=True)
    _assert_call(got, ref, plan, action, agent, what)
    _assert_engines(e, twin, what)
    assert not bool(div.any()), (what, "the loop's own replicas differ", div.tolist())
    assert got.mpc.planned == 10 == agent.draw and horizons == [H] * 10 and agent.syncs == 1
    assert bool((got.plan.planned == 10.0).all()) and bool((got.plan.idle == 0.0).all()) and bool((got.steps == 10).all())
    # a group's replicas carry equal rows: the caller reads every R-th
    assert torch.equal(_bits(got.stats[..., COLS]), _bits(got.stats[:, lead][..., COLS])) and torch.equal(_bits(got.returns), _bits(got.returns[lead]))
    s = got.plan.summary()
    assert np.allclose(s["per_env"]["action_frequency"].sum(-1), 1.0) and np.array_equal(s["planned"], np.full(G, 10))
    assert np.array_equal(s["diverged"], np.zeros(G)) and s["per_env"]["mean_score"].shape == (G,)
    assert bool((got.plan.gain >= 0.0).all())      # the incumbent's score never falls from one iteration to the next


def test_the_chunked_output_block_changes_nothing():
    import torch
    G, R = 3, 8
    twin, agent, ref, plan, action, _, _ = _reference(G, R, True)
    e = _engine(G * R, debug_flags=L.PLAN_DEBUG_TWO_STEPS)
    got = _call(e, 10, R, sync=True)
    _assert_call(got, ref, plan, action, agent, "two-step block")
    _assert_engines(e, twin, "two-step block")
    nostats = _call(_engine(G * R), 10, R, sync=True, plan_stats=False)
    assert nostats.plan is None and torch.equal(_bits(nostats.returns), _bits(ref.returns)) and nostats.mpc.planned == 10
    assert torch.equal(nostats.mpc.step_actions, action)


def test_continuation_with_into_and_the_returned_arrays_and_act_behind_rollout_stats():
    import torch
    G, R = 3, 8
    N = G * R
    twin, agent, ref, plan, action, _, _ = _reference(G, R, True)
    e = _engine(N)
    first = _call(e, 5, R, sync=True)
    assert first.mpc.steps == H and first.mpc.planned == 5
    got = _call(e, 5, R, into=first, probs=first.mpc.probs, best_seq=first.mpc.best_seq, resume_steps=first.mpc.steps, draw=first.mpc.planned)
    assert got is first
    _assert_call(got, ref, plan, action, agent, "5 + 5")
    _assert_engines(e, twin, "5 + 5")
    # the agent's own call, split 3 + 4 + 3, and then act() on both sides
    e2, mine = _engine(N), _agent(R)
    st = mine.rollout_stats(e2, 3)
    st = mine.rollout_stats(e2, 4, into=st)
    st = mine.rollout_stats(e2, 3, into=st)
    _assert_call(st, ref, plan, action, agent, "agent 3 + 4 + 3")
    assert (mine.draw, mine.last_horizon, mine._step, mine.syncs) == (agent.draw, agent.last_horizon, agent._step, 1) and mine.last is None
    twin2, theirs = _engine(N), _agent(R)
    _loop(twin2, theirs, 10)
    a, b = mine.act(e2), theirs.act(twin2)
    assert torch.equal(a, b) and mine.draw == theirs.draw == 11 and mine.syncs == theirs.syncs == 1
    assert torch.equal(_bits(mine.last.probs), _bits(theirs.last.probs)) and torch.equal(mine.last.best_seq, theirs.last.best_seq)
    assert torch.equal(_bits(mine.last.best_score), _bits(theirs.last.best_score))
    e2.step(a), twin2.step(b)
    _assert_engines(e2, twin2, "the step behind act()")


def _replicas_equal_their_leaders(e, R, what):
    """inside one engine: every replica's rows of the state arrays (but those that depend on which re-centring request found which slot:
    tests/test_gpu_mark.py SCHEDULED) and of the single-step views against its group's first env's, bit for bit"""
    import torch
    N = e.n_envs
    lead = np.arange(N) // R * R
    for k, x in _grab(e).items():
        if k in SCHEDULED:
            continue
        same = np.array_equal(x[:, lead], x) if k in ("qcum_t", "hist_t") else np.array_equal(x[lead], x)
        assert same, (what, k)
    tl = torch.as_tensor(lead, device=e.device)
    for nm in ("obs", "share_obs", "rew", "done", "info"):
        u = getattr(e, nm).clone()
        if nm == "info":
            u[:, RSV] = 0
        assert torch.equal(u, u[tl]), (what, nm)


def test_the_episodes_end_inside_the_call_and_the_call_after_it():
    import torch
    G, R = 3, 8
    N = G * R
    e, twin = _engine(N), _engine(N)
    g = torch.Generator(device="cpu").manual_seed(9)
    acts = torch.randint(0, 3, (EP - 7, N, 3), generator=g, dtype=torch.int32).to(e.device)
    e.rollout_stats(acts), twin.rollout_stats(acts)
    assert e.steps_to_episode_end() == 7
    agent, mine = _agent(R), _agent(R)
    ref, plan, action, horizons, div = _loop(twin, agent, 7)
    got = mine.rollout_stats(e, 7)
    _assert_call(got, ref, plan, action, agent, "to the episode's end")
    _assert_engines(e, twin, "to the episode's end")
    assert horizons == [4, 4, 4, 3, 2, 1, 0] == [d[0] for d in mpc_schedule(7, 7, H, True)] and not bool(div.any())
    assert e.steps_to_episode_end() == EP and bool(e.done.bool().all())      # the auto-reset is inside the call
    assert bool((got.plan.idle == 1.0).all()) and bool((got.plan.planned == 6.0).all())
    assert got.mpc.planned == 6 and got.mpc.steps == 0 and mine.draw == agent.draw == 6 and mine.syncs == agent.syncs == 1
    idle = torch.tensor(IDLE, dtype=torch.int32, device=e.device)
    assert torch.equal(got.mpc.step_actions, idle.expand(N, 3)) and torch.equal(got.mpc.best_action, idle.expand(G, 3))
    assert mine._probs is None and mine.last_horizon == 0
    lead = torch.arange(N, device=e.device) // R * R
    assert not torch.equal(e.obs, e.obs[lead])      # the replicas drew resets of their own
    # the next call syncs again and starts fresh, in the new episode
    ref, plan, action, horizons, div = _loop(twin, agent, 3)
    got = mine.rollout_stats(e, 3)
    _assert_call(got, ref, plan, action, agent, "the call after the reset")
    _assert_engines(e, twin, "the call after the reset")
    assert mine.draw == 9 and bool((got.plan.idle == 0.0).all()) and mine.syncs == agent.syncs == 2 and horizons == [H] * 3
    _replicas_equal_their_leaders(e, R, "the call after the reset")


def test_a_forecast_a_limit_and_a_terminal_term_apply_to_every_decision():
    import torch
    G, R = 3, 8
    e, twin = _engine(G * R), _engine(G * R)
    for x in (e, twin):
        x.set_plan_terms(limits={"dc_int_temperature": (None, 24.0, 1.5)}, terminal={"ls_tasks_in_queue": -0.002})
    kw = dict(forecast="persistence", gamma=0.95, reward_weights=(1.0, 0.5, 2.0), info_weights={"bat_CO2_footprint": -1e-3})
    agent, mine = _agent(R, **kw), _agent(R, **kw)
    ref, plan, action, _, _ = _loop(twin, agent, 6)
    got = mine.rollout_stats(e, 6)
    assert e.plan_forecast["carbon"] == "persistence"
    _assert_call(got, ref, plan, action, agent, "forecast and terms")
    _assert_engines(e, twin, "forecast and terms")
    # ... and they matter: the same steps without them are planned differently
    plain = _call(_engine(G * R), 6, R, sync=True)
    assert not torch.equal(_bits(plain.plan.sums), _bits(got.plan.sums))


class _FixedDc(GroupCEMMPCAgent):
    """the agent with agent_dc's action fixed to 1 in every sampled replica"""

    def _plan(self, env, K, **kw):
        return super()._plan(env, K, fixed_action=(-1, 1, -1), **kw)


def test_a_fixed_action_alpha_and_p_min():
    G, R = 3, 8
    e, twin = _engine(G * R), _engine(G * R)
    agent = _agent(R, _FixedDc, alpha=0.3, p_min=0.05)
    ref, plan, action, _, _ = _loop(twin, agent, 6)
    got = _call(e, 6, R, dict(alpha=0.3, p_min=0.05), fixed_action=(-1, 1, -1), sync=True)
    _assert_call(got, ref, plan, action, agent, "fixed action")
    _assert_engines(e, twin, "fixed action")
    assert bool((got.plan.action_counts[:, 1, 1] == 6).all())      # agent_dc held its set-point throughout


def test_the_agreement_check_counts_a_perturbed_replica_and_nothing_else():
    """After a sync, one plain step in which replica 2 of group 1 discharges while its group idles; then 6 steps WITHOUT a sync.  The
    reference is the twin's loop of plan_cem_groups and GroupCEMMPCAgent.shifted directly -- no agent, so nothing syncs --, and `diverged`
    restated on the host from the twin's views after every step."""
    import torch
    G, R = 5, 6      # group 1 is envs 6 .. 11: its first env and the perturbed one, env 8, sit in different wavefronts of the check
    N, odd = G * R, R + 2
    e, twin = _engine(N), _engine(N)
    x = torch.tensor(IDLE, dtype=torch.int32, device=e.device).expand(N, 3).contiguous()
    x[odd, 2] = 0      # the battery's other action
    for eng in (e, twin):
        eng.sync_groups(R)
        eng.step(x)
    probs = seq = ref = None
    counts, sums = _plan_arrays(G, twin.device)
    div = torch.zeros((G,), dtype=torch.int32, device=twin.device)
    for t in range(6):
        res = twin.plan_cem_groups(R, H, I, E, probs=probs, best_seq=seq, seed=CEM["seed"], draw=t)
        ref = twin.rollout_stats(res.step_actions[None], into=ref)
        _fold(counts, sums, res.action, res.best_score)
        div += _host_diverged(twin, R)
        probs, seq = GroupCEMMPCAgent.shifted(res.probs, res.best_seq, H)
    got = _call(e, 6, R, sync=False)
    print("diverged", got.plan.diverged.tolist(), "restated", div.tolist())
    assert torch.equal(got.plan.diverged, div), (got.plan.diverged.tolist(), div.tolist())
    assert int(div[1]) > 0 and not bool(div[[0, 2, 3, 4]].any()), div.tolist()
    assert np.array_equal(got.plan.summary()["diverged"], div.cpu().numpy())
    # ... and everything else of the call equals the loop's
    assert torch.equal(_bits(got.stats[..., COLS]), _bits(ref.stats[..., COLS])) and torch.equal(_bits(got.returns), _bits(ref.returns))
    assert torch.equal(got.plan.counts, counts) and torch.equal(_bits(got.plan.sums), _bits(sums))
    assert torch.equal(_bits(got.mpc.probs), _bits(res.probs)) and torch.equal(got.mpc.best_seq, res.best_seq)
    assert torch.equal(got.mpc.step_actions, res.step_actions) and torch.equal(got.mpc.best_action, res.action)
    _assert_engines(e, twin, "a perturbed replica")
    # a second call accumulates on what `into` holds; one without starts from 0
    more = _call(e, 1, R, sync=False, into=got, probs=got.mpc.probs, best_seq=got.mpc.best_seq, resume_steps=got.mpc.steps, draw=6)
    assert int(more.plan.diverged[1]) > int(div[1]) and int(more.plan.diverged[0]) == 0
    anew = _call(e, 1, R, sync=False, draw=7)
    assert 0 < int(anew.plan.diverged[1]) <= R - 1 and int(anew.plan.diverged[0]) == 0
    # a sync puts the group back: nothing is counted any more
    assert not bool(_call(e, 2, R, sync=True, draw=8).plan.diverged.any())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
RN, RR = 8, 4      # the refusal engines: two groups of four


def _raw(e, keep, n_steps=2, accumulate=0, null_mpc=False, mpc=None, cem=None, null=(), offset=None, objective=None):
    """sdc_rollout_cem_groups_stats on e through ctypes: valid arguments but for what is asked for -- `mpc`: fields of
    sdc_mpc_group_params, `cem`: fields of its sdc_cem_group_params, `null`: arrays passed as NULL, `offset`: array -> bytes its address
    is moved by; ValueError(the message) on -2.  `keep`: the caller's dict the arrays are put into (they hold 7s)"""
    import torch
    N, dev = e.n_envs, e.device
    G = N // RR
    shapes = dict(stats=((4, N, L.INFO_DIM), torch.float64), returns=((N, 3), torch.float64), counts=((N, 2), torch.int32),
                  plan_counts=((G, 3, 5), torch.int32), plan_sums=((G, 4), torch.float64), diverged=((G,), torch.int32),
                  probs=((H, G, 3, 3), torch.float64), best_seq=((H, G, 3), torch.int32), best_score=((I, G), torch.float64),
                  best_action=((G, 3), torch.int32), step_actions=((N, 3), torch.int32), cand=((H, N, 3), torch.int32),
                  cand_score=((N,), torch.float64))
    for nm, (shape, dtype) in shapes.items():
        keep[nm] = torch.full((int(np.prod(shape)) + 4,), 7, dtype=dtype, device=dev)      # (room for a moved address)
    p = L.SdcMpcGroupParams()
    p.horizon, p.warm_start, p.resume, p.resume_steps, p.sync_first = H, 1, 0, 0, 0
    p.idle_action[:] = IDLE
    p.cem.group_size, p.cem.group_base, p.cem.n_iters, p.cem.n_elite, p.cem.seed = RR, 0, I, E, 77
    p.cem.fixed_action[:] = [-1, -1, -1]
    for k, v in (mpc or {}).items():
        if k == "idle_action":
            p.idle_action[:] = v
        else:
            setattr(p, k, v)
    for k, v in (cem or {}).items():
        if k == "fixed_action":
            p.cem.fixed_action[:] = v
        else:
            setattr(p.cem, k, v)
    ptr = lambda nm: None if nm in null else C.c_void_p(keep[nm].data_ptr() + (offset or {}).get(nm, 0))
    outs = dict(obs=e.obs, share_obs=e.share_obs, rew=e.rew, done=e.done, info=e.info, final_obs=e.final_obs)
    optr = lambda nm: None if nm in null else C.c_void_p(outs[nm].data_ptr() + (offset or {}).get(nm, 0))
    torch.cuda.synchronize()
    rc = e.lib.sdc_rollout_cem_groups_stats(e._h, n_steps, None if null_mpc else C.byref(p), objective, accumulate,
                                            *[ptr(nm) for nm in shapes], *[optr(nm) for nm in outs], e._stream())
    assert rc == -2, rc
    torch.cuda.synchronize()
    for nm in shapes:
        assert bool((keep[nm] == 7).all()), nm      # the caller's arrays: untouched
    raise ValueError(e.lib.sdc_last_error().decode())


def _objective(gamma):
    o = L.SdcPlanObjective()
    o.reward_weight[:] = [1.0, 1.0, 1.0]
    o.gamma = gamma
    return o


def test_refusals_leave_the_engine_the_launch_counter_and_the_arrays_untouched():
    import torch
    from tests.plan_util import objective, refusal_engines
    N, R = RN, RR
    a, b, split, fresh, verify, late = refusal_engines(N, alongside=2)      # a, b, split: 38 steps left of 48; late: 2 left, no auto-reset
    mask = np.zeros(N, dtype=np.uint8)
    mask[5] = 1
    split.reset(mask=mask)      # env 5 starts a new episode: group 1 is out of step
    keep = {}
    raw = lambda match, eng=a, **kw: refused(eng, match, lambda: _raw(eng, keep, **kw))
    # sdc_rollout_stats' own, but for `actions`
    raw("n_steps = 0 must be positive", n_steps=0)
    raw("null array", null=("stats",))
    raw("null array", null=("share_obs",))
    raw("stats / returns not 16-byte aligned", offset={"returns": 8})
    raw("not dword-aligned", offset={"counts": 2})
    raw("accumulate = 2", accumulate=2)
    raw("sdc_reset must be called first", eng=fresh)
    raw("verify mode", eng=verify)
    raw("past the end of an episode", n_steps=39)
    raw("past the end of an episode", n_steps=39, mpc=dict(sync_first=1))
    raw("past the end of an episode", eng=late, n_steps=3)
    # the loop's parameters
    raw("null mpc", null_mpc=True)
    raw("horizon = 0 outside", mpc=dict(horizon=0))
    raw("horizon = 257 outside", mpc=dict(horizon=L.MARK_MAX_STEPS + 1))
    raw("warm_start = 2", mpc=dict(warm_start=2))
    raw("resume = -1", mpc=dict(resume=-1))
    raw("resume_steps = 0 outside", mpc=dict(resume=1, resume_steps=0))
    raw("resume_steps = 5 outside", mpc=dict(resume=1, resume_steps=H + 1))
    raw(r"idle_action\[2\] = 3", mpc=dict(idle_action=[1, 1, 3]))
    raw(r"idle_action\[0\] = -1", mpc=dict(idle_action=[-1, 1, 2]))
    raw("sync_first = 2 outside", mpc=dict(sync_first=2))
    raw("sync_first = -1 outside", mpc=dict(sync_first=-1))
    raw("sync_first with resume", mpc=dict(sync_first=1, resume=1, resume_steps=2))
    # sdc_plan_cem_groups' parameters, objective and arrays
    for field, bad, match in (("n_iters", 0, "n_iters"), ("iter0", -1, "iter0"), ("iter0", 65535, "iter0"), ("group_size", 1, "group_size"),
                              ("group_size", 0, "group_size"), ("group_size", L.CEM_MAX_GROUP + 1, "group_size"),
                              ("group_size", 3, "not a multiple"), ("group_size", 16, "not a multiple"), ("n_elite", 0, "n_elite"),
                              ("n_elite", R + 1, "n_elite"), ("group_base", -1, "group_base"), ("alpha", 1.0, "alpha"),
                              ("alpha", -0.1, "alpha"), ("p_min", 0.5, "p_min"), ("p_min", float("nan"), "p_min")):
        raw(match, cem={field: bad})
    raw(r"fixed_action\[1\] = 3", cem=dict(fixed_action=(-1, 3, -1)))
    for nm in ("probs", "best_seq", "best_score", "best_action", "step_actions", "cand", "cand_score"):
        raw("null array", null=(nm,))
    raw("gamma", objective=C.byref(_objective(gamma=0.0)))
    raw("gamma", objective=C.byref(_objective(gamma=1.5)))
    raw("n_cols", objective=C.byref(objective(L.PLAN_MAX_COLS + 1, 0)))
    raw("info column", objective=C.byref(objective(1, L.INFO_DIM)))
    # the plan statistics -- all three or none -- and the alignments
    for some in (("plan_counts",), ("plan_sums",), ("diverged",), ("plan_counts", "plan_sums"), ("plan_sums", "diverged"),
                 ("plan_counts", "diverged")):
        raw("given together or not at all", null=some)
    raw("plan_sums not 16-byte aligned", offset={"plan_sums": 8})
    raw("plan_counts / diverged not dword-aligned", offset={"plan_counts": 2})
    raw("plan_counts / diverged not dword-aligned", offset={"diverged": 2})
    raw("not 8-byte aligned", offset={"probs": 4})
    raw("not 8-byte aligned", offset={"cand_score": 4})
    raw("not dword-aligned", offset={"best_seq": 2})
    raw("not dword-aligned", offset={"step_actions": 2})
    raw("not dword-aligned", offset={"obs": 2})
    # a group out of step: refused without a sync (with one the clone establishes it: the call at the end of this test)
    raw("out of step.*env 5.*episode step", eng=split)
    # a forecast whose values are too short for the longest decision
    a.set_plan_forecast(carbon="values", values=torch.zeros((H + 1, N, 4), dtype=torch.float64, device=a.device))
    raw("entries")
    a.set_plan_forecast()
    # the order of the refusals: of two faults at once the earlier one is named
    raw("n_steps = 0 must be positive", n_steps=0, null_mpc=True)
    raw("horizon = 0 outside", mpc=dict(horizon=0), cem=dict(n_iters=0))
    raw("n_iters = 0", cem=dict(n_iters=0), null=("probs",))
    raw("null array", null=("probs",), offset={"plan_sums": 8})
    raw("plan_sums not 16-byte aligned", offset={"plan_sums": 8}, objective=C.byref(_objective(gamma=0.0)))
    raw("gamma", objective=C.byref(_objective(gamma=0.0)), n_steps=39)
    raw("sync_first = 2 outside", mpc=dict(sync_first=2), cem=dict(n_iters=0))
    raw("not a multiple", cem=dict(group_size=3, alpha=1.0))
    split.set_plan_forecast(carbon="values", values=torch.zeros((H + 1, N, 4), dtype=torch.float64, device=split.device))
    raw("out of step", eng=split)
    split.set_plan_forecast()
    # through the binding: ValueError before the library is asked, or from it
    call = lambda **kw: (lambda: _call(a, kw.pop("n", 2), kw.pop("R", R), **kw))
    G = N // R
    refused(a, "three integers", call(idle_action=(1, 1)))
    refused(a, "three integers", call(fixed_action=(1, 1)))
    refused(a, "resuming needs probs and best_seq", call(resume_steps=2))
    refused(a, "must not be negative", call(resume_steps=-1))
    refused(a, "probs", call(probs=torch.zeros((H, N, 3, 3), dtype=torch.float64, device=a.device)))      # per env, not per group
    refused(a, "best_seq", call(best_seq=torch.ones((H - 1, G, 3), dtype=torch.int32, device=a.device)))
    refused(a, "at most 8", call(info_weights={k: 1.0 for k in L.INFO_COLS[:9]}))
    refused(a, "horizon = 300", lambda: a.rollout_cem_groups_stats(2, R, 300, I, E))
    refused(a, "group_size = 1 outside", call(R=1))
    refused(a, "not a multiple", call(R=3))
    refused(a, "sync_first with resume", call(sync=True, resume_steps=2, probs=torch.zeros((H, G, 3, 3), dtype=torch.float64, device=a.device),
                                              best_seq=torch.ones((H, G, 3), dtype=torch.int32, device=a.device)))
    refused(a, "exactly when plan_stats", call(into=a.rollout_stats(torch.ones((1, N, 3), dtype=torch.int32, device=a.device))))
    b.rollout_stats(torch.ones((1, N, 3), dtype=torch.int32, device=a.device))
    per_env = a.rollout_cem_stats(1, H, I, 4, E)      # a per-env PlanStats is not a per-group one
    b.rollout_cem_stats(1, H, I, 4, E)
    refused(a, "into.plan must be a PlanStats of this engine", call(into=per_env))
    # the launch counter: the twin that was refused nothing runs the loop, the refused engine the call -- the same bits
    agent = _agent(R)
    ref, plan, action, _, _ = _loop(b, agent, 3)
    got = _call(a, 3, R, sync=True)
    _assert_call(got, ref, plan, action, agent, "behind the refusals")
    _assert_engines(a, b, "behind the refusals")
    # the group that was out of step: the sync puts it back, and the call goes through to the end of the leaders' episode
    assert split.steps_to_episode_end() == 38      # (seven envs are 10 steps in, env 5 none)
    done = _call(split, 38, R, sync=True)
    assert bool((done.steps == 38).all()) and done.mpc.planned == 37 and not bool(done.plan.diverged.any())
    assert split.steps_to_episode_end() == 48 and bool(split.done.bool().all())


# ---- the vector env ---------------------------------------------------------------------------------------------------------------
ARGS = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True}


def _vec(N, **extra):
    return SustainDCVecEnv(dict(ARGS, **extra), n_envs=N, seed=3, months=[6] * N, return_torch=True)


def _same_bits(x, y, what):
    import torch
    assert torch.equal(_bits(x.stats[..., COLS]), _bits(y.stats[..., COLS])), (what, "stats")
    assert torch.equal(_bits(x.returns), _bits(y.returns)) and torch.equal(x.counts, y.counts), (what, "returns / counts")
    assert torch.equal(x.plan.counts, y.plan.counts) and torch.equal(_bits(x.plan.sums), _bits(y.plan.sums)), (what, "plan")
    assert torch.equal(x.plan.diverged, y.plan.diverged), (what, "diverged")


def test_vec_env_evaluate_with_the_group_planner_the_subset_refusal_and_a_deepcopy():
    import torch
    G, R, EPS = 3, 4, 2
    N = G * R
    a, b = _vec(N), _vec(N)
    assert a.episode_steps == EP
    with pytest.raises(ValueError, match="call reset"):
        a.rollout_cem_groups_stats(2, R, H, I, E, sync=True)
    mine = _agent(R)
    got = a.evaluate(EPS, mpc=mine)
    assert got.stats.shape == (EPS, 4, N, L.INFO_DIM) and got.returns.shape == (EPS, N, 3) and got.counts.shape == (EPS, N, 2)
    assert isinstance(got.plan, PlanStats) and got.plan.counts.shape == (EPS, G, 3, 5) and got.plan.sums.shape == (EPS, G, 4)
    assert got.plan.diverged.shape == (EPS, G) and not bool(got.plan.diverged.any())
    assert got.policy is None and bool((got.steps == EP).all()) and mine.syncs == EPS      # one call per episode, each with a sync
    assert bool((got.plan.planned == EP - 1.0).all()) and bool((got.plan.idle == 1.0).all())
    s = got.plan.summary()
    assert s["per_env"]["mean_score"].shape == (EPS, G) and s["batch"]["action_frequency"].shape == (EPS, 3, 3) and s["diverged"].shape == (EPS, G)
    # ... equals two single calls from a reset, the agent's draw counter running on
    b.reset()
    theirs = _agent(R)
    for ep in range(EPS):
        one = theirs.rollout_stats(b, EP)
        _same_bits(EpisodeStats(got.stats[ep], got.returns[ep], got.counts[ep],
                                plan=PlanStats(got.plan.counts[ep], got.plan.sums[ep], got.plan.diverged[ep])), one, f"episode {ep}")
    assert theirs.draw == EPS * (EP - 1) == mine.draw and theirs.syncs == EPS
    _same_state(a.engine, b.engine, "evaluate against two calls")
    _same_out(a.engine, b.engine, "evaluate against two calls")
    for bad in (dict(actors=True), dict(actions=torch.ones((EP, N, 3), dtype=torch.int32))):
        with pytest.raises(ValueError, match="neither actions nor actors"):
            a.evaluate(1, mpc=_agent(R), **bad)
    # an agent subset: the other slots' stepped actions would differ from the planner's best_action
    sub = _vec(4, agents=["agent_dc", "agent_bat"])
    sub.reset()
    with pytest.raises(ValueError, match="best_action"):
        sub.rollout_cem_groups_stats(2, 2, H, I, E, sync=True)
    with pytest.raises(ValueError, match="all three agents"):
        sub.evaluate(1, mpc=_agent(2))
    sub.close()
    # a copy of the env afterwards evaluates identically
    c = copy.deepcopy(a)
    x, y = a.evaluate(1, mpc=_agent(R, seed=5)), c.evaluate(1, mpc=_agent(R, seed=5))
    _same_bits(x, y, "the copy's evaluate")
    for v in (a, b, c):
        v.close()
