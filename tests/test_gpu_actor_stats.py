"""Policy evaluation on the device (SdcEngine.rollout_actor_stats / evaluate(actors=True), SustainDCVecEnv.set_actor / rollout_actor_stats /
evaluate over sdc_rollout_actor_stats) held to the call's stated arithmetic (include/sustaindc_hip.h).

THE REFERENCE throughout is a twin engine with the same seed and the same actors that runs `rollout_actor(K, sample, want_logits=True)` and
materialises everything: its rew / info go through tests/test_gpu_stats.py's `_restate`, its actions / logits through `_policy_restate`
below -- the header's policy arithmetic in torch fp64, one tensor op per operation, in step order.

THE BARS: environment statistics, the policy counts and LAST: every bit.  LOGP and ENTROPY: |got - ref| <= 1e-12 * sum_k |term_k| -- two
fp64 libraries' exp / log differ by about 4e-16 on this arithmetic and an fp32 evaluation by about 7e-9 (both checked on the CPU with 672
steps of logits of scale 2.5), so 1e-12 sits more than three orders from each; the observed maximum is printed.  Between two device runs:
every bit of everything.  info[reserved] is left out between two engines, as in tests/test_gpu_stats.py.  No case is excluded from any
comparison: the actions compared are the twin kernel's own, so near-tied logits need no filter.

 1. the arithmetic at 6 envs (18 lanes: one partial wavefront of sdc_policy_stats_kernel) and 130 (390 lanes: full wavefronts and a partial
    one), by the mode and by a draw; the engine's state and single-step views against the twin's;  2. the chunked output block (chunks of
    2, 2, 2, 1 steps: SWITCHES and LAST across chunk boundaries), and policy_stats=False;  3. continuation with `into=`;  4. the episode's
    end with auto-reset, and the call after it;  5. four envs per wavefront: by debug flag at 132 envs, by size at 8 192;  6. the refusals,
    each of which leaves the engine untouched;  7. `evaluate` through the vector env;  8. copy.deepcopy of a vector env with actors.

96-step episodes, rings of 128 keys."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import EpisodeStats, PolicyStats, SustainDCVecEnv, dc_config, traces
from dc_rl_amd.engine import SdcEngine
from tests.plan_util import refused
from tests.test_gpu_actor import _torch_actor
from tests.test_gpu_mark import _same_out, _same_state
from tests.test_gpu_stats import _assert_stats, _bits, _restate

pytestmark = pytest.mark.gpu

EP, CAP, K7 = 96, 128, 7
RSV = L.INFO_IDX["reserved"]
COLS = [c for c in range(L.INFO_DIM) if c != RSV]
PAIR_KERNEL, QUAD_KERNEL = "sdc_rollout_actor_kernel", "sdc_rollout_actor_quad_kernel"
REL = 1e-12


@functools.lru_cache(maxsize=None)
def _nets(activation="tanh", base=100):
    return tuple(_torch_actor(base + a, activation) for a in range(3))


def _engine(N, seed=5, debug_flags=0, actors="tanh", reset=True):
    """tests/test_gpu_actor.py's engine with rings of CAP keys; `actors`: the activation of the three nets set before the reset (None:
    no actor set)"""
    tb = traces.synthetic_tables("ny", 0)
    p = dc_config.size_datacenter("dc_config.json", 1, 30.0)
    e = SdcEngine(N, episode_steps=EP, auto_reset=True, seed=seed, debug_flags=debug_flags, hist_cap=CAP)
    e.set_tables(0, tb["W"], tb["C"], tb["T"], tb["WB"])
    e.set_dc_params(0, p)
    e.assign(0, 0, 174, 188)
    if actors is not None:
        _set_actors(e, actors)
    if reset:
        e.reset()
    return e


def _set_actors(e, activation="tanh", slots=(0, 1, 2)):
    for a in slots:
        sd = dict(_nets(activation)[a].state_dict())
        sd["activation"] = activation
        e.set_actor(a, sd)


def _policy_restate(acts, logits):
    """sdc_rollout_actor_stats' policy arithmetic from actions [K, N, 3] / logits [K, N, 3, 3], one step at a time in step order, one
    tensor op per operation -> (counts [N, 3, 5] int32, sums [N, 3, 2] float64, sum_k |term_k| [N, 3, 2])"""
    import torch
    K, N = acts.shape[0], acts.shape[1]
    dev = acts.device
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    n, sw, last = torch.zeros((N, 3, 3), **i32), torch.zeros((N, 3), **i32), torch.full((N, 3), -1, **i32)
    logp, ent, alogp, aent = (torch.zeros((N, 3), **f64) for _ in range(4))
    which = torch.arange(3, **i32)
    for k in range(K):
        j = acts[k]
        n = n + (j[..., None] == which).to(torch.int32)
        sw = sw + ((last >= 0) & (j != last)).to(torch.int32)
        last = j.clone()
        l = logits[k]
        m = torch.maximum(torch.maximum(l[..., 0], l[..., 1]), l[..., 2])      # fp32
        z = l.double() - m.double()[..., None]
        e = torch.exp(z)
        s = (e[..., 0] + e[..., 1]) + e[..., 2]
        lse = torch.log(s)
        lp = z - lse[..., None]
        p = e / s[..., None]
        lpj = torch.gather(lp, -1, j.long()[..., None])[..., 0]
        h = -((p[..., 0] * lp[..., 0] + p[..., 1] * lp[..., 1]) + p[..., 2] * lp[..., 2])
        logp, ent = logp + lpj, ent + h
        alogp, aent = alogp + lpj.abs(), aent + h.abs()
    counts = torch.cat([n, sw[..., None], last[..., None]], -1).contiguous()
    return counts, torch.stack([logp, ent], -1).contiguous(), torch.stack([alogp, aent], -1)


def _assert_policy(ps, want, what):
    """a PolicyStats against _policy_restate's tuple: the counts to the bit, the two sums within REL * sum_k |term_k|"""
    import torch
    assert isinstance(ps, PolicyStats)
    counts, sums, bound = want
    N = counts.shape[0]
    assert ps.counts.shape == (N, 3, L.POLICY_COUNTS) and ps.counts.dtype == torch.int32 and ps.counts.is_cuda
    assert ps.sums.shape == (N, 3, L.POLICY_SUMS) and ps.sums.dtype == torch.float64
    assert ps.action_counts.shape == (N, 3, 3) and ps.switches.shape == (N, 3) and ps.last_action.shape == (N, 3)
    if not torch.equal(ps.counts, counts):
        bad = (ps.counts != counts).nonzero()
        raise AssertionError((what, "counts", len(bad), bad[:4].tolist()))
    err = (ps.sums - sums).abs()
    ratio = float((err / bound).max())
    print(f"{what}: max |got - ref| / sum|term| over LOGP and ENTROPY = {ratio:.3e} (bar {REL:.0e}), max |got - ref| = {float(err.max()):.3e}")
    assert bool((bound > 0).all()), (what, "a sum of |terms| is zero")
    assert bool((err <= REL * bound).all()), (what, "sums", ratio)


def _assert_same_bits(x, y, what):
    """two device runs' EpisodeStats: every bit of everything but info[reserved]"""
    import torch
    assert torch.equal(_bits(x.stats[..., COLS]), _bits(y.stats[..., COLS])), (what, "stats")
    assert torch.equal(_bits(x.returns), _bits(y.returns)) and torch.equal(x.counts, y.counts), (what, "returns / counts")
    assert torch.equal(x.policy.counts, y.policy.counts), (what, "policy counts")
    assert torch.equal(_bits(x.policy.sums), _bits(y.policy.sums)), (what, "policy sums")


def _materialise(a, K, sample):
    """the twin's K steps: rollout_actor's outputs and their two restatements"""
    obs, share, rew, done, info, acts, logits = a.rollout_actor(K, sample=sample, want_logits=True)
    return dict(rew=rew, info=info, acts=acts, logits=logits, want=_restate(rew, info), pol=_policy_restate(acts, logits))


@functools.lru_cache(maxsize=None)
def _reference(N, sample):
    """the K7-step run every test at N envs shares: a twin's materialised `rollout_actor` and its restatements -- computed once, never
    written to"""
    a = _engine(N)
    ref = _materialise(a, K7, sample)
    ref["twin"] = a
    ref["views"] = {nm: getattr(a, nm).clone() for nm in ("obs", "share_obs", "rew", "done")}
    return ref


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("N", [6, 130])
def test_arithmetic_against_the_twins_materialised_rollout(N, sample):
    import torch
    ref = _reference(N, sample)
    b = _engine(N)
    st = b.rollout_actor_stats(K7, sample=sample)
    _assert_stats(st, ref["want"], f"N = {N}, sample = {sample}")
    _assert_policy(st.policy, ref["pol"], f"N = {N}, sample = {sample}")
    assert bool((st.steps == K7).all()) and not bool(st.fault.any())
    ps = st.policy
    assert bool((ps.action_counts.sum(-1) == K7).all())
    assert torch.equal(ps.last_action, ref["acts"][-1]) and torch.equal(ps.logp, ps.sums[..., 0]) and torch.equal(ps.entropy, ps.sums[..., 1])
    assert bool((ps.logp < 0).all()) and bool((ps.entropy > 0).all())
    if sample:      # the result is not trivial
        played = (ps.action_counts.sum(0) > 0).sum(-1)      # [3 agents]: different actions played somewhere in the batch
        assert bool((played >= 2).all()), played.tolist()
        assert 0 < int(ps.switches.sum()) < (K7 - 1) * N * 3
    # the engine moved as the twin did: every state field, and the single-step views follow the last step
    a = ref["twin"]
    _same_state(a, b, f"rollout_actor_stats against rollout_actor, N = {N}, sample = {sample}")
    _same_out(a, b, f"the views after rollout_actor_stats, N = {N}, sample = {sample}")
    for nm, x in ref["views"].items():
        assert torch.equal(getattr(b, nm), x), nm
    assert b.last_step_kernel() == a.last_step_kernel() == PAIR_KERNEL
    s = ps.summary()
    assert s["per_env"]["action_frequency"].shape == (N, 3, 3) and np.array_equal(s["steps"], np.full((N, 3), K7))
    assert np.array_equal(s["per_env"]["switch_rate"], ps.switches.cpu().numpy() / (K7 - 1.0))
    b.close()


def test_chunked_output_block_gives_the_same_bits():
    N = 130
    ref = _reference(N, True)
    b = _engine(N)
    c = _engine(N, debug_flags=L.PLAN_DEBUG_TWO_STEPS)      # (chunks of 2, 2, 2, 1 steps)
    sb, sc = b.rollout_actor_stats(K7, sample=True), c.rollout_actor_stats(K7, sample=True)
    _assert_stats(sc, ref["want"], "chunked")
    _assert_policy(sc.policy, ref["pol"], "chunked")
    _assert_same_bits(sb, sc, "chunked against unchunked")
    _same_state(ref["twin"], c, "chunked rollout_actor_stats against rollout_actor")
    _same_out(ref["twin"], c, "the views after the chunked call")
    assert c.last_step_kernel() == PAIR_KERNEL
    # without the policy arrays: the environment's statistics alone
    d = _engine(N, debug_flags=L.PLAN_DEBUG_TWO_STEPS)
    sd = d.rollout_actor_stats(K7, sample=True, policy_stats=False)
    assert sd.policy is None
    _assert_stats(sd, ref["want"], "chunked, policy_stats=False")
    _same_state(ref["twin"], d, "policy_stats=False against rollout_actor")
    for e in (b, c, d):
        e.close()


def test_continuation_with_into_equals_one_call():
    import torch
    N = 130
    ref = _reference(N, True)
    b, whole = _engine(N), _engine(N)
    one = whole.rollout_actor_stats(K7, sample=True)
    first = b.rollout_actor_stats(3, sample=True)
    _assert_stats(first, _restate(ref["rew"][:3], ref["info"][:3]), "the first 3 steps")
    _assert_policy(first.policy, _policy_restate(ref["acts"][:3], ref["logits"][:3]), "the first 3 steps")
    ptrs = [x.data_ptr() for x in (first.stats, first.returns, first.counts, first.policy.counts, first.policy.sums)]
    again = b.rollout_actor_stats(4, sample=True, into=first)
    assert again is first      # ... updated in place
    assert ptrs == [x.data_ptr() for x in (first.stats, first.returns, first.counts, first.policy.counts, first.policy.sums)]
    _assert_stats(first, ref["want"], "3 + 4 steps")
    _assert_policy(first.policy, ref["pol"], "3 + 4 steps")
    _assert_same_bits(first, one, "3 + 4 steps against 7 in one call")
    pol = first.policy
    mismatched = [
        EpisodeStats(first.stats[:, :N - 1], first.returns, first.counts, pol),                                   # wrong shape
        EpisodeStats(first.stats, first.returns, first.counts, PolicyStats(pol.counts[:N - 1], pol.sums)),
        EpisodeStats(first.stats, first.returns, first.counts, PolicyStats(pol.counts, pol.sums.float())),
        EpisodeStats(first.stats.cpu(), first.returns.cpu(), first.counts.cpu(), pol),                            # not this engine's device
        EpisodeStats(first.stats, first.returns, first.counts, PolicyStats(pol.counts.cpu(), pol.sums.cpu())),
        EpisodeStats(first.stats, first.returns, first.counts),                                                   # no PolicyStats
    ]
    if torch.cuda.device_count() > 1:      # another engine's device
        mismatched.append(EpisodeStats(first.stats, first.returns, first.counts, PolicyStats(pol.counts.to("cuda:1"), pol.sums.to("cuda:1"))))
    for bad in mismatched:
        refused(b, "into", lambda: b.rollout_actor_stats(1, sample=True, into=bad))
    refused(b, "PolicyStats", lambda: b.rollout_actor_stats(1, sample=True, into=mismatched[5]))
    refused(b, "PolicyStats", lambda: b.rollout_actor_stats(1, sample=True, into=first, policy_stats=False))
    b.close()
    whole.close()


def test_episode_end_with_auto_reset_and_the_call_after_it():
    import torch
    N = 130
    a, b = _engine(N), _engine(N)
    for e in (a, b):
        e.rollout_actor(20, sample=True)
    K = b.steps_to_episode_end()
    assert K == EP - 20 and b.config["auto_reset"]
    ref = _materialise(a, K, True)
    st = b.rollout_actor_stats(K, sample=True)
    _assert_stats(st, ref["want"], "to the episode's end")
    _assert_policy(st.policy, ref["pol"], "to the episode's end")
    assert bool((st.steps == K).all()) and bool((st.policy.action_counts.sum(-1) == K).all())      # (the terminal step included)
    assert bool((b.done == 1).all()) and torch.equal(b.final_obs, a.final_obs)
    assert torch.equal(b.obs, a.obs) and torch.equal(b.share_obs, a.share_obs)      # (the reset observations)
    assert not torch.equal(b.obs, b.final_obs)
    assert b.steps_to_episode_end() == EP == a.steps_to_episode_end()
    _same_state(a, b, "after the auto-reset")
    # the next episode's first steps, a fresh result: the observation latch survived the reset
    nxt = _materialise(a, 5, True)
    s2 = b.rollout_actor_stats(5, sample=True)
    _assert_stats(s2, nxt["want"], "5 steps into the next episode")
    _assert_policy(s2.policy, nxt["pol"], "5 steps into the next episode")
    assert bool((s2.steps == 5).all())
    _same_state(a, b, "5 steps into the next episode")
    _same_out(a, b, "the views 5 steps into the next episode")
    a.close()
    b.close()


def test_four_envs_per_wavefront_by_flag_and_by_size():
    import torch
    N = 132
    q, p = _engine(N, debug_flags=L.DEBUG_QUAD), _engine(N)
    sq, sp = q.rollout_actor_stats(K7, sample=True), p.rollout_actor_stats(K7, sample=True)
    assert q.last_step_kernel() == QUAD_KERNEL and p.last_step_kernel() == PAIR_KERNEL
    _assert_same_bits(sq, sp, "DEBUG_QUAD against two envs per wavefront, N = 132")
    _same_state(p, q, "DEBUG_QUAD against two envs per wavefront, N = 132")
    q.close()
    p.close()
    N, K = 8192, 12      # csrc/sdc_dispatch.hpp SDC_QUAD_MIN_ENVS_LOOP: four envs per wavefront by size
    a, b = _engine(N), _engine(N)
    ref = _materialise(a, K, True)
    st = b.rollout_actor_stats(K, sample=True)
    assert a.last_step_kernel() == QUAD_KERNEL == b.last_step_kernel()
    _assert_stats(st, ref["want"], "8 192 envs")
    _assert_policy(st.policy, ref["pol"], "8 192 envs")
    _same_out(a, b, "the views at 8 192 envs")
    assert a.steps_to_episode_end() == b.steps_to_episode_end() == EP - K
    a.close()
    b.close()


def test_refusals_name_their_reason_and_leave_the_engine_untouched():
    import torch
    N = 8
    a = _engine(N)
    a.rollout_actor(10, sample=True)      # 86 steps left
    missing = _engine(N, actors=None)
    _set_actors(missing, slots=(0, 2))
    mixed = _engine(N, actors=None)
    _set_actors(mixed, "tanh", slots=(0, 1))
    _set_actors(mixed, "relu", slots=(2,))
    mixed.reset()
    late = _engine(N, actors=None)        # actors set after the last reset: no observation latch
    _set_actors(late)
    fresh = _engine(N, reset=False)
    verify = _engine(N, debug_flags=L.DEBUG_VERIFY)
    odd = _engine(7)

    refused(missing, "sdc_set_actor all three", lambda: missing.rollout_actor_stats(2))
    refused(mixed, "share one activation", lambda: mixed.rollout_actor_stats(2))
    refused(late, "no observations yet", lambda: late.rollout_actor_stats(2))
    refused(a, "must be positive", lambda: a.rollout_actor_stats(0))
    refused(a, "past the end of an episode", lambda: a.rollout_actor_stats(87))
    refused(fresh, "sdc_reset must be called first", lambda: fresh.rollout_actor_stats(2))
    refused(verify, "verify mode", lambda: verify.rollout_actor_stats(2))
    refused(odd, "common case", lambda: odd.rollout_actor_stats(2))
    refused(a, "must be positive", lambda: a.evaluate(0, actors=True))
    refused(a, "give no actions", lambda: a.evaluate(1, torch.ones((EP, N, 3), dtype=torch.int32, device=a.device), actors=True))
    # what the Python surface cannot send: straight to the library
    f64 = torch.zeros(4 * N * L.INFO_DIM + 2, dtype=torch.float64, device=a.device)
    ret = torch.zeros(N * 3 + 2, dtype=torch.float64, device=a.device)
    cnt = torch.zeros((N, 2), dtype=torch.int32, device=a.device)
    pc = torch.zeros((N, 3, L.POLICY_COUNTS), dtype=torch.int32, device=a.device)
    psm = torch.zeros(N * 3 * L.POLICY_SUMS + 2, dtype=torch.float64, device=a.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    assert f64.data_ptr() % 16 == 0 and ret.data_ptr() % 16 == 0 and psm.data_ptr() % 16 == 0

    def raw(eng=a, n_steps=2, sample=0, accumulate=0, stats=f64, returns=ret, counts=cnt, pcounts=pc, psums=psm, h=True):
        rc = eng.lib.sdc_rollout_actor_stats(eng._h if h else None, n_steps, sample, accumulate, p(stats), p(returns), p(counts), p(pcounts),
                                             p(psums), p(eng.obs), p(eng.share_obs), p(eng.rew), p(eng.done), p(eng.info), p(eng.final_obs),
                                             eng._stream())
        eng._refused(rc)

    refused(a, "null handle", lambda: raw(h=False))
    for bad in (-1, 2):
        refused(a, "sample", lambda: raw(sample=bad))
        refused(a, "accumulate", lambda: raw(accumulate=bad))
    refused(a, "together", lambda: raw(psums=None))
    refused(a, "together", lambda: raw(pcounts=None))
    refused(a, "policy_sums not 16-byte aligned", lambda: raw(psums=psm[1:]))      # (off by 8 bytes)
    refused(a, "not 16-byte aligned", lambda: raw(stats=f64[1:]))
    refused(a, "null array", lambda: raw(counts=None))
    refused(a, "must be positive", lambda: raw(n_steps=-2))
    refused(a, "past the end of an episode", lambda: raw(n_steps=87))
    # ... and the calls next to them go through: both policy arrays, neither, a whole remaining episode
    raw()
    raw(pcounts=None, psums=None, accumulate=1)
    torch.cuda.synchronize()
    assert cnt[:, 0].tolist() == [4] * N and pc[:, :, :3].sum(-1).tolist() == [[2] * 3] * N and a.steps_to_episode_end() == 82
    st = a.rollout_actor_stats(82)
    assert bool((st.steps == 82).all()) and a.steps_to_episode_end() == EP and bool((a.done == 1).all())
    for e in (a, missing, mixed, late, fresh, verify, odd):
        e.close()


ARGS = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True}


def _vec(N, **extra):
    return SustainDCVecEnv(dict(ARGS, **extra), n_envs=N, seed=3, months=[6] * N, return_torch=True)


def test_vec_env_evaluate_with_the_actors():
    import torch
    N, E = 40, 2
    a, b = _vec(N), _vec(N)
    assert a.episode_steps == EP
    nets = _nets()
    for v in (a, b):
        v.set_actor("agent_ls", nets[0].state_dict())
        v.set_actor(1, nets[1].state_dict())
        v.set_actor("agent_bat", nets[2].state_dict())
    with pytest.raises(ValueError, match="unknown agent"):
        a.set_actor("agent_x", nets[0].state_dict())
    with pytest.raises(ValueError, match="slot"):
        a.set_actor(3, nets[0].state_dict())
    with pytest.raises(ValueError, match="reset"):
        a.rollout_actor_stats(2)
    a.accumulate_logger_sums()
    logged = a.read_logger_sums(reset=False)
    st = a.evaluate(E, actors=True, sample=True)
    assert a.read_logger_sums(reset=False) == logged      # the accumulator counts what went through step(): untouched
    assert st.stats.shape == (E, 4, N, L.INFO_DIM) and st.returns.shape == (E, N, 3) and st.counts.shape == (E, N, 2)
    assert st.policy.counts.shape == (E, N, 3, L.POLICY_COUNTS) and st.policy.sums.shape == (E, N, 3, L.POLICY_SUMS)
    # the twin: a reset, then two materialised episodes of its engine (the auto-reset between them)
    eng = b.engine
    eng.reset()
    for e in range(E):
        ref = _materialise(eng, EP, True)
        assert bool(ref["rew"].shape[0] == EP) and eng.steps_to_episode_end() == EP
        _assert_stats(EpisodeStats(st.stats[e], st.returns[e], st.counts[e]), ref["want"], f"episode {e}")
        _assert_policy(PolicyStats(st.policy.counts[e], st.policy.sums[e]), ref["pol"], f"episode {e}")
    assert bool((st.steps == EP).all()) and not bool(st.fault.any())
    assert not torch.equal(st.policy.counts[0], st.policy.counts[1])      # two different episodes
    s, ps = st.summary(), st.policy.summary()
    assert s["per_env"]["average_CO2_footprint"].shape == (E, N) and ps["per_env"]["switch_rate"].shape == (E, N, 3)
    assert ps["batch"]["action_frequency"].shape == (E, 3, 3) and np.allclose(ps["batch"]["action_frequency"].sum(-1), 1.0)
    # the envs stand at the start of a fresh episode; rollout_actor_stats goes on from there, in step with the twin
    assert not a._need_reset and a.engine.steps_to_episode_end() == EP
    ref = _materialise(eng, 5, False)
    s5 = a.rollout_actor_stats(5)
    _assert_stats(s5, ref["want"], "5 steps after evaluate")
    _assert_policy(s5.policy, ref["pol"], "5 steps after evaluate")
    assert a.read_logger_sums(reset=False) == logged
    # without actors: what evaluate returned before -- the do-nothing baseline (ls 1, dc 1, bat 2), policy None
    base = a.evaluate(1)
    assert base.policy is None and base.stats.shape == (1, 4, N, L.INFO_DIM)
    eng.reset()
    nothing = torch.tensor([1, 1, 2], dtype=torch.int32, device=eng.device).expand(EP, N, 3).contiguous()
    o = eng.rollout(nothing)
    _assert_stats(EpisodeStats(base.stats[0], base.returns[0], base.counts[0]), _restate(o[2], o[4]), "evaluate without actors")
    with pytest.raises(ValueError, match="give no actions"):
        a.evaluate(1, torch.ones((EP, N, 3), dtype=torch.int32), actors=True)
    a.close()
    b.close()
    # an env that trains an agent subset has no place for three actors
    sub = _vec(4, agents=["agent_dc", "agent_bat"])
    with pytest.raises(ValueError, match="all three agents"):
        sub.set_actor("agent_dc", nets[1].state_dict())
    with pytest.raises(ValueError, match="sdc_set_actor all three"):
        sub.evaluate(1, actors=True)
    sub.close()


def test_deepcopy_of_a_vec_env_carries_the_actors():
    import torch
    N = 40
    a = _vec(N)
    for slot, net in enumerate(_nets()):
        a.set_actor(slot, net.state_dict())
    a.reset()
    a.rollout_actor_stats(9, sample=True)
    c = copy.deepcopy(a)
    assert sorted(c.engine._actors) == [0, 1, 2]
    x, y = a.rollout_actor_stats(8, sample=True), c.rollout_actor_stats(8, sample=True)      # the rest of the episode they share ...
    _assert_same_bits(x, y, "the copy's next 8 steps")
    x, y = a.evaluate(1, actors=True, sample=True), c.evaluate(1, actors=True, sample=True)  # ... and one from a reset
    _assert_same_bits(x, y, "the copy's evaluate")
    assert bool((x.steps == EP).all())
    a.close()
    c.close()
