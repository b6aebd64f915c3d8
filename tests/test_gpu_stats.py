"""Episode statistics on the device (SdcEngine.rollout_stats / evaluate, SustainDCVecEnv.rollout_stats / evaluate over sdc_rollout_stats)
held to the call's stated arithmetic (include/sustaindc_hip.h) restated in torch fp64 from a twin engine's `rollout` outputs, bit for bit
through an int64 view.

 1. the arithmetic at 3 envs (one partial wavefront of the reduce kernel) and 130 (32 full wavefronts and a partial one): all four fields
    of the info columns, returns, steps, fault; the engine's state and single-step views against the twin's;  2. the chunked output block
    (debug_flags PLAN_DEBUG_TWO_STEPS: chunks of 2, 2, 2, 1 steps);  3. continuation with `into=`;  4. the episode's end with auto-reset;  5. built-in
    policies on all three slots;  6. fault bits;  7. the large-batch rollout path (12 288 envs);  8. the refusals, each of which leaves
    the engine untouched;  9. `evaluate` through the vector env against a per-step step() loop.

ONE COLUMN IS NOT COMPARED BETWEEN TWO ENGINES: info[reserved] says how a step's reward state was served and is "scheduling-dependent,
unlike every other output" (include/sustaindc_hip.h), so two engines on one trajectory may differ in it (tests/test_gpu_mark.py _same_out
leaves it out for the same reason).  Its reduction is checked within ONE engine instead: a one-step call's sum, min and max of every
column, reserved included, are the bits of the engine's own info view of that step.

NOT in verify mode, for the reason tests/test_gpu_plan.py gives: sdc_rollout refuses it, and so does this call (test 8).  96-step episodes,
rings of 128 keys."""
import ctypes as C
import functools

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import EpisodeStats, SustainDCVecEnv
from tests.plan_util import EP, RSV, _twins, refusal_engines, refused
from tests.test_gpu_mark import _mk, _same_out, _same_state

pytestmark = pytest.mark.gpu

K7 = 7
FAULT = L.INFO_IDX["fault"]
COLS = [c for c in range(L.INFO_DIM) if c != RSV]
FAULT_ACTION = 64      # include/sustaindc_hip.h SDC_FAULT_ACTION


def _seq(K, N, g):
    import torch
    return torch.randint(0, 3, (K, N, 3), dtype=torch.int32, generator=g).cuda()


def _restate(rew, info):
    """sdc_rollout_stats' arithmetic from rew [K, N, 3] / info [K, N, 44], one step at a time in step order -> (stats [4, N, 44],
    returns [N, 3], steps [N], fault [N])"""
    import torch
    K, N = rew.shape[0], rew.shape[1]
    kw = dict(dtype=torch.float64, device=rew.device)
    s, npos, ret = torch.zeros((N, L.INFO_DIM), **kw), torch.zeros((N, L.INFO_DIM), **kw), torch.zeros((N, 3), **kw)
    lo, hi = torch.full((N, L.INFO_DIM), float("inf"), **kw), torch.full((N, L.INFO_DIM), float("-inf"), **kw)
    steps, fault = torch.zeros(N, dtype=torch.int32, device=rew.device), torch.zeros(N, dtype=torch.int64, device=rew.device)
    one, zero = torch.ones((), **kw), torch.zeros((), **kw)
    for k in range(K):
        x = info[k].double()
        s = s + x
        lo = torch.where(x < lo, x, lo)
        hi = torch.where(x > hi, x, hi)
        npos = npos + torch.where(x > 0.0, one, zero)
        ret = ret + rew[k].double()
        steps = steps + 1
        fault = fault | info[k][:, FAULT].to(torch.int64)
    return torch.stack([s, lo, hi, npos]), ret, steps, fault.to(torch.int32)


def _bits(x):
    import torch
    return x.contiguous().view(torch.int64)


def _assert_stats(st, want, what):
    """an EpisodeStats against _restate's tuple: every bit of the four fields of every column but info[reserved], of the returns, the
    steps and the fault bits"""
    import torch
    assert isinstance(st, EpisodeStats)
    stats, ret, steps, fault = want
    N = ret.shape[0]
    assert st.stats.shape == (4, N, L.INFO_DIM) and st.stats.dtype == torch.float64 and st.stats.is_cuda
    assert st.returns.shape == (N, 3) and st.returns.dtype == torch.float64
    assert st.steps.shape == (N,) and st.fault.shape == (N,) and st.counts.dtype == torch.int32
    for f, nm in enumerate(("sum", "min", "max", "n_pos")):
        got, ref = getattr(st, nm)[:, COLS], stats[f][:, COLS]
        assert getattr(st, nm).data_ptr() == st.stats[f].data_ptr()
        if not torch.equal(_bits(got), _bits(ref)):
            bad = (_bits(got) != _bits(ref)).nonzero()
            raise AssertionError((what, nm, len(bad), bad[:4].tolist()))
    assert torch.equal(_bits(st.returns), _bits(ret)), (what, "returns")
    assert torch.equal(st.steps, steps), (what, "steps")
    assert torch.equal(st.fault, fault), (what, "fault")


@functools.lru_cache(maxsize=None)
def _reference(N):
    """the K7-step run every test at N envs shares: the action sequence, a twin's `rollout` outputs of it and their restatement --
    computed once, never written to"""
    (a,), g = _twins(N, n=1)
    acts = _seq(K7, N, g)
    o = a.rollout(acts)
    rew, info = o[2].clone(), o[4].clone()
    views = {nm: getattr(a, nm).clone() for nm in ("obs", "share_obs", "rew", "done", "info")}
    return dict(acts=acts, rew=rew, info=info, want=_restate(rew, info), twin=a, views=views)


@pytest.mark.parametrize("N", [3, 130])
def test_arithmetic_bit_for_bit_against_the_twins_rollout(N):
    import torch
    ref = _reference(N)
    (b,), _ = _twins(N, n=1)
    st = b.rollout_stats(ref["acts"])
    _assert_stats(st, ref["want"], f"N = {N}")
    assert bool((st.steps == K7).all()) and not bool(st.fault.any())
    # the statistics are not trivial: columns move within 7 steps, some values are positive and some are not
    assert bool((st.max > st.min).any()) and bool((st.n_pos == K7).any()) and bool((st.n_pos == 0).any())
    assert torch.equal(st.col("dc_water_usage"), st.sum[:, L.INFO_IDX["dc_water_usage"]])
    # the engine moved as the twin did: every state field, and the single-step views follow the last step
    a = ref["twin"]
    _same_state(a, b, f"rollout_stats against rollout, N = {N}")
    _same_out(a, b, f"the views after rollout_stats, N = {N}")
    for nm, x in ref["views"].items():
        if nm != "info":
            assert torch.equal(getattr(b, nm), x), nm
    assert b.last_step_kernel() == a.last_step_kernel()
    # one more step, within ONE engine: sum, min and max of every column -- info[reserved] included -- are the step's own info row
    nxt = _seq(1, N, torch.Generator(device="cpu").manual_seed(N))
    one = b.rollout_stats(nxt)
    x = b.info.double()
    assert torch.equal(_bits(one.sum), _bits(x + 0.0))      # (0.0 + -0.0 is +0.0)
    assert torch.equal(_bits(one.min), _bits(x)) and torch.equal(_bits(one.max), _bits(x))
    assert torch.equal(one.n_pos, (x > 0).double()) and torch.equal(_bits(one.returns), _bits(b.rew.double() + 0.0))
    assert bool((one.steps == 1).all())
    b.close()


def test_chunked_output_block_gives_the_same_bits():
    N = 130
    ref = _reference(N)
    (c,), _ = _twins(N, n=1, debug_flags=L.PLAN_DEBUG_TWO_STEPS)      # (chunks of 2, 2, 2, 1 steps)
    _assert_stats(c.rollout_stats(ref["acts"]), ref["want"], "chunked")
    _same_state(ref["twin"], c, "chunked rollout_stats against rollout")
    _same_out(ref["twin"], c, "the views after the chunked call")
    c.close()


def test_continuation_with_into_equals_one_call():
    import torch
    N = 130
    ref = _reference(N)
    (b,), _ = _twins(N, n=1)
    first = b.rollout_stats(ref["acts"][:3])
    _assert_stats(first, _restate(ref["rew"][:3], ref["info"][:3]), "the first 3 steps")
    again = b.rollout_stats(ref["acts"][3:], into=first)
    assert again is first
    _assert_stats(first, ref["want"], "3 + 4 steps")
    with pytest.raises(ValueError, match="into must be"):
        b.rollout_stats(ref["acts"][:1], into=EpisodeStats(first.stats[:, :N - 1], first.returns, first.counts))
    with pytest.raises(ValueError, match="into must be"):
        b.rollout_stats(ref["acts"][:1], into=EpisodeStats(first.stats.float(), first.returns, first.counts))
    b.close()


def test_episode_end_with_auto_reset():
    import torch
    N = 130
    (a, b), g = _twins(N)
    K = b.steps_to_episode_end()
    assert K == EP - 20 and b.config["auto_reset"]
    acts = _seq(K, N, g)
    o = a.rollout(acts)
    st = b.rollout_stats(acts)
    _assert_stats(st, _restate(o[2], o[4]), "to the episode's end")
    assert bool((st.steps == K).all())
    assert bool((b.done == 1).all()) and torch.equal(b.final_obs, a.final_obs)
    assert torch.equal(b.obs, a.obs) and torch.equal(b.share_obs, a.share_obs)      # (the reset observations)
    assert not torch.equal(b.obs, b.final_obs)
    assert b.steps_to_episode_end() == EP == a.steps_to_episode_end()
    _same_state(a, b, "after the auto-reset")
    a.close()
    b.close()


def test_built_in_policies_on_all_three_slots():
    import torch
    N = 130
    (a, b), _ = _twins(N, policy=(1, 3, 2))      # ls do-nothing, dc trim-and-respond, bat rule-based (include/sustaindc_hip.h sdc_policy)
    o = a.rollout_policy(K7)
    st = b.rollout_stats(n_steps=K7)
    _assert_stats(st, _restate(o[2], o[4]), "built-in policies")
    assert o[5].shape == (K7, N, 3)      # (the actions the policies chose: the info rows hold them as bat_action / dc_crac_setpoint_delta)
    _same_state(a, b, "rollout_stats against rollout_policy")
    with pytest.raises(ValueError, match="n_steps"):
        b.rollout_stats()
    a.close()
    b.close()


def test_fault_bits_are_the_or_over_the_steps():
    import torch
    N = 130
    (a, b), g = _twins(N)
    acts = _seq(K7, N, g)
    pairs = [(0, 1), (3, 5), (2, 5), (6, 129)]      # (step, env): an agent_dc action outside {0, 1, 2}, played as "do nothing"
    for k, e in pairs:
        acts[k, e, 1] = 7
    o = a.rollout(acts)
    st = b.rollout_stats(acts)
    want = torch.zeros(N, dtype=torch.int32, device=b.device)
    want[[e for _, e in pairs]] = FAULT_ACTION
    assert torch.equal(st.fault, want), st.fault.nonzero().flatten().tolist()
    _assert_stats(st, _restate(o[2], o[4]), "fault bits")
    a.close()
    b.close()


def test_large_batch_rollout_path_every_env():
    N, K = 12288, 3      # csrc/sdc_dispatch.hpp SDC_WIDE_ROLLOUT_MIN_ENVS: a rollout is K launches of the lane-per-env kernel
    (a, b), g = _twins(N, history=4)
    assert a.last_step_kernel() == "sdc_dynamics_wide_kernel"
    acts = _seq(K, N, g)
    o = a.rollout(acts)
    st = b.rollout_stats(acts)
    assert b.last_step_kernel() == "sdc_dynamics_wide_kernel" == a.last_step_kernel()
    _assert_stats(st, _restate(o[2], o[4]), "12 288 envs")
    _same_out(a, b, "the views at 12 288 envs")
    assert a.steps_to_episode_end() == b.steps_to_episode_end()
    a.close()
    b.close()


def test_refusals_name_their_reason_and_leave_the_engine_untouched():
    import torch
    N = 8
    a, fresh, verify, late = refusal_engines(N)
    pol = _mk(N, ep=48, policy=(1, 3, 2))
    ones = lambda K, n=N: torch.ones((K, n, 3), dtype=torch.int32, device=a.device)

    # through the Python surface
    refused(a, "actions must be", lambda: a.rollout_stats(ones(2, N + 1)))
    refused(a, "actions must be", lambda: a.rollout_stats(ones(2).long()))
    refused(a, "actions must be", lambda: a.rollout_stats(ones(2).cpu()))
    refused(a, "actions must be", lambda: a.rollout_stats(ones(4)[::2]))
    refused(a, "n_steps does not match", lambda: a.rollout_stats(ones(2), n_steps=3))
    refused(a, "built-in policy", lambda: a.rollout_stats(n_steps=2))
    refused(a, "must be positive", lambda: a.rollout_stats(ones(0)))
    refused(a, "past the end of an episode", lambda: a.rollout_stats(ones(39)))      # (38 steps left)
    refused(late, "past the end of an episode", lambda: late.rollout_stats(ones(3)))
    refused(fresh, "sdc_reset must be called first", lambda: fresh.rollout_stats(ones(2)))
    refused(verify, "verify mode", lambda: verify.rollout_stats(ones(2)))
    refused(a, "must be positive", lambda: a.evaluate(0))
    refused(a, "built-in policy", lambda: a.evaluate(1))
    # what the Python surface cannot send: straight to the library
    x = ones(2)
    f64 = torch.zeros(4 * N * L.INFO_DIM + 2, dtype=torch.float64, device=a.device)
    ret = torch.zeros(N * 3 + 2, dtype=torch.float64, device=a.device)
    cnt = torch.zeros((N, 2), dtype=torch.int32, device=a.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    assert f64.data_ptr() % 16 == 0 and ret.data_ptr() % 16 == 0

    def raw(eng=a, n_steps=2, acts=x, accumulate=0, stats=f64, returns=ret, counts=cnt, obs=True, share=True, h=True):
        rc = eng.lib.sdc_rollout_stats(eng._h if h else None, n_steps, p(acts), accumulate, p(stats), p(returns), p(counts),
                                       p(eng.obs) if obs else None, p(eng.share_obs) if share else None, p(eng.rew), p(eng.done),
                                       p(eng.info), p(eng.final_obs), eng._stream())
        eng._refused(rc)

    refused(a, "null handle", lambda: raw(h=False))
    refused(a, "must be positive", lambda: raw(n_steps=0))
    refused(a, "must be positive", lambda: raw(n_steps=-2))
    refused(a, "past the end of an episode", lambda: raw(n_steps=39, acts=ones(39)))
    for nm in ("stats", "returns", "counts"):
        refused(a, "null array", lambda: raw(**{nm: None}))
    refused(a, "null array", lambda: raw(obs=False))
    refused(a, "null array", lambda: raw(share=False))
    refused(a, "not 16-byte aligned", lambda: raw(stats=f64[1:]))
    refused(a, "not 16-byte aligned", lambda: raw(returns=ret[1:]))
    for bad in (-1, 2):
        refused(a, "accumulate", lambda: raw(accumulate=bad))
    refused(a, "actions may only be NULL", lambda: raw(acts=None))
    refused(fresh, "sdc_reset must be called first", lambda: raw(eng=fresh))
    refused(verify, "verify mode", lambda: raw(eng=verify))
    # ... and the calls next to them go through: built-in policies without actions, the last steps of an episode without auto-reset,
    # a whole remaining episode
    raw(eng=pol, acts=None)
    torch.cuda.synchronize()
    assert cnt[:, 0].tolist() == [2] * N and pol.steps_to_episode_end() == 46
    st = late.rollout_stats(ones(2))
    assert bool((st.steps == 2).all()) and late.steps_to_episode_end() == 0 and bool((late.done == 1).all())
    refused(late, "past the end of an episode", lambda: late.rollout_stats(ones(1)))
    assert bool((a.rollout_stats(ones(38)).steps == 38).all()) and a.steps_to_episode_end() == 48
    for e in (a, fresh, verify, late, pol):
        e.close()


def test_vec_env_evaluate_against_a_step_loop():
    import torch
    N, E = 130, 2
    args = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True,
            "agents": ["agent_dc", "agent_bat"]}      # agent_ls is played on the device; the trained agents do nothing: dc 1, bat 2
    a = SustainDCVecEnv(args, n_envs=N, seed=3, months=[6] * N, return_torch=True)
    b = SustainDCVecEnv(args, n_envs=N, seed=3, months=[6] * N, return_torch=True)
    assert a.episode_steps == EP
    with pytest.raises(ValueError, match="reset"):
        a.rollout_stats(n_steps=2)
    a.accumulate_logger_sums()
    a.reset()
    nothing = torch.tensor([1, 2], dtype=torch.int32, device=a.engine.device).expand(N, 2).contiguous()
    a.step(nothing)
    logged = a.read_logger_sums(reset=False)
    with pytest.raises(ValueError, match="shape"):
        a.evaluate(1, torch.ones((EP, N, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="episode_steps"):
        a.evaluate(1, torch.ones((EP - 1, N, 2), dtype=torch.int32))
    st = a.evaluate(E)
    assert a.read_logger_sums(reset=False) == logged      # the accumulator counts what went through step(): untouched
    assert st.stats.shape == (E, 4, N, L.INFO_DIM) and st.returns.shape == (E, N, 3) and st.counts.shape == (E, N, 2)
    # the twin: two resets (a's own and evaluate's), then a step() loop reduced per env in fp64 in step order
    b.reset()
    b.step(nothing)
    b.reset()
    want = np.zeros((E, 4, N, L.INFO_DIM))
    ret = np.zeros((E, N, 3))
    for e in range(E):
        s, npos = np.zeros((N, L.INFO_DIM)), np.zeros((N, L.INFO_DIM))
        lo, hi = np.full((N, L.INFO_DIM), np.inf), np.full((N, L.INFO_DIM), -np.inf)
        for k in range(EP):
            done = b.step(nothing)[3]
            x = b.engine.info.cpu().numpy().astype(np.float64)
            s = s + x
            lo, hi = np.where(x < lo, x, lo), np.where(x > hi, x, hi)
            npos = npos + np.where(x > 0.0, 1.0, 0.0)
            ret[e] = ret[e] + b.engine.rew.cpu().numpy().astype(np.float64)
            assert bool(done.all()) == (k == EP - 1)
        want[e] = np.stack([s, lo, hi, npos])
    got = st.stats.cpu().numpy()
    assert np.array_equal(got[:, :, :, COLS].view(np.int64), want[:, :, :, COLS].view(np.int64))
    assert np.array_equal(st.returns.cpu().numpy().view(np.int64), ret.view(np.int64))
    assert bool((st.steps == EP).all()) and not bool(st.fault.any())
    assert not np.array_equal(got[0], got[1])      # two different episodes
    # the envs stand at the start of a fresh episode, in step with the twin
    for u, v in zip(a.step(nothing)[:4], b.step(nothing)[:4]):
        assert torch.equal(u, v)
    s = st.summary()
    c = L.INFO_IDX["bat_CO2_footprint"]
    assert s["per_env"]["average_CO2_footprint"].shape == (E, N) and s["batch"]["total_water_usage"].shape == (E,)
    assert np.array_equal(s["per_env"]["average_CO2_footprint"], want[:, 0, :, c] / EP)
    # rollout_stats with explicit actions in the env's agent order equals the engine's with the third slot filled
    acts = torch.randint(0, 3, (5, N, 2), dtype=torch.int32, generator=torch.Generator().manual_seed(1)).cuda()
    full = torch.ones((5, N, 3), dtype=torch.int32, device=acts.device)
    full[..., 1:] = acts
    stepped = a.read_logger_sums(reset=False)      # (the step() above went through the accumulator, as it should: two steps by now)
    assert stepped[1] == logged[1] + 1 and stepped[0] != logged[0]
    ra, rb = a.rollout_stats(acts), b.engine.rollout_stats(full)
    assert torch.equal(_bits(ra.stats[:, :, COLS]), _bits(rb.stats[:, :, COLS])) and torch.equal(ra.returns, rb.returns)
    assert a.read_logger_sums(reset=False) == stepped      # ... and rollout_stats leaves it alone as well
    a.close()
    b.close()
