"""The actors on stored rows, on the device (sdc_actor_evaluate, sdc_ppo_terms; SdcEngine.actor_logits, evaluate_actions, ppo_terms,
actor_update_terms), at 40 envs:
  1. logits: every row count around a wavefront's 16 and a workgroup's 64 rows, dense and strided rows, dense and strided logits, the
     four networks of the fixture the reference wrote -- against the reference's logits and a torch fp64 forward, 2e-4 (the project's
     bar for these actors, tests/test_gpu_actor.py);
  2. a row's logits do not depend on where the row stands: by bits, in a call large enough for a second pass of every workgroup;
     a strided store leaves the floats between the rows alone;
  3. against the closed loop: `evaluate_actions` over a collected batch stays within 2e-4 of the rollout kernel's logits (which sums in
     another order), is the same bits twice, so that an unchanged actor has ratio exactly 1, approx_kl 0, clip_frac 0;
  4. `ppo_terms` against tests/ppo_ref.py: ratio and surr within one fp32 ulp and at most one in a thousand different at all, the factor
     and the statistics bit for bit from the device's own stored outputs;
  5. the HAPPO loop over the agents in the order 2, 0, 1 with the factor carried along; the vector env's delegates; copy.deepcopy;
  6. every refusal reaches Python as a ValueError with the header's text, and nothing is launched behind it."""
import copy

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import actor_eval_ref as AE
from tests import actor_ref as AR
from tests import critic_ref as CR
from tests import onpolicy_ref as OR
from tests import ppo_ref as PR
from tests.plan_util import refused

pytestmark = pytest.mark.gpu

N = 40
BAR = 2e-4
POISON = np.array([OR.NAN_BITS], dtype=np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def eng():
    e = AR.engine(N, False)
    yield e
    e.close()


def _poisoned(torch, n, device):
    return torch.full((n,), OR.NAN_BITS, dtype=torch.int32, device=device).view(torch.float32)


def _is_poison(x):
    import torch
    return bool((x.contiguous().view(torch.int32) == OR.NAN_BITS).all())


def _eval(e, agent, rows, stride, ls, tail=7):
    """sdc_actor_evaluate of `rows` (a device tensor [R, 26]) placed `stride` floats apart in a poisoned buffer (at the agent's place
    of an [R][3][26] array when stride is 78) into a poisoned logits buffer `ls` floats apart (at the agent's column of [R][3][3] when
    ls is 9) with `tail` poisoned floats behind it -> logits [R, 3]; everything else in the logits buffer must still be poison"""
    import torch
    R = rows.shape[0]
    off = 26 * agent if stride == 78 else 0
    lo = 3 * agent if ls == 9 else 0
    buf = _poisoned(torch, R * stride, e.device).view(R, stride)
    buf[:, off:off + 26] = rows
    out = _poisoned(torch, R * ls + tail, e.device)
    e._behind_torch_stream()
    e._actor_evaluate(agent, buf, off, stride, R, out, lo, ls)
    body = out[:R * ls].view(R, ls)
    got = body[:, lo:lo + 3].clone()
    keep = torch.ones(ls, dtype=torch.bool, device=e.device)
    keep[lo:lo + 3] = False
    assert _is_poison(body[:, keep]) and _is_poison(out[R * ls:]), (R, stride, ls)
    return got


# ---- 1. logits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,feature_norm", AE.CONFIGS)
def test_logits_against_the_fixture_and_torch_fp64(eng, activation, feature_norm):
    import torch
    c = AE.case(activation, feature_norm)
    for slot in range(3):
        eng.set_actor(slot, AE.params(activation, feature_norm))
    net = AE.torch_net(activation, feature_norm)
    obs = torch.from_numpy(c["obs"])
    with torch.no_grad():
        ref64 = copy.deepcopy(net).double()(obs.double()).numpy()
        ref32 = net(obs).numpy()
    assert np.abs(ref64 - c["logits"]).max() <= BAR        # (the fixture's network is the one loaded)
    dev_obs = obs.to(eng.device)
    worst = 0.0
    for i, R in enumerate((1, 15, 16, 17, 63, 64, 65, AE.R)):
        for stride in (26, 78):
            for ls in (3, 9):
                agent = (i + stride + ls) % 3
                got = _eval(eng, agent, dev_obs[:R], stride, ls).cpu().numpy()
                err = max(np.abs(got - c["logits"][:R]).max(), np.abs(got - ref64[:R]).max())
                worst = max(worst, float(err))
                assert err <= BAR, (R, stride, ls, err)
    # the public forms give the raw call's bits
    dense = eng.actor_logits(1, dev_obs)
    assert dense.shape == (AE.R, 3) and torch.equal(dense, _eval(eng, 1, dev_obs, 26, 3))
    three = torch.zeros((AE.R, 3, 26), device=eng.device)
    three[:, 2] = dev_obs
    assert torch.equal(eng.actor_logits(2, three), dense) and torch.equal(eng.actor_logits(0, three.view(1, AE.R, 3, 26))[0], eng.actor_logits(0, three))
    assert eng.actor_logits(0, dev_obs.view(AE.R, 1, 26)).shape == (AE.R, 1, 3)
    print("%s: sdc_actor_evaluate max |logit error| %.2e against the reference's logits and torch fp64; torch fp32 against fp64 on the same "
          "rows %.2e" % (AE.cfg_name(activation, feature_norm), worst, np.abs(ref32 - ref64).max()))


# ---- 2. row independence -------------------------------------------------------------------------------------------------------------------
def test_a_rows_logits_do_not_depend_on_its_place(eng):
    import torch
    for slot, (activation, fn) in enumerate((("tanh", True), ("tanh", False), ("tanh", True))):
        eng.set_actor(slot, AE.params(activation, fn))
    n = L.ACTOR_EVAL_MAX_BLOCKS * 64 + 17      # every workgroup's first pass, one workgroup's second, a last tile of one row
    g = torch.Generator().manual_seed(11)
    rows = torch.randn((n, 26), generator=g).to(eng.device)
    rows[1::3, 14:] = 0.0
    big = eng.actor_logits(0, rows)
    assert big.shape == (n, 3) and bool(torch.isfinite(big).all())
    chunks = torch.cat([eng.actor_logits(0, rows[i:i + 64].contiguous()) for i in range(0, n, 64)])
    assert torch.equal(big.view(torch.int32), chunks.view(torch.int32))
    # the same rows at another position, another stride, alone
    for i in (0, 15, 16, 63, 64, 4097, 65535, 65536, n - 1):
        alone = eng.actor_logits(0, rows[i:i + 1].contiguous())
        assert torch.equal(alone[0].view(torch.int32), big[i].view(torch.int32)), i
    shifted = eng.actor_logits(0, rows[5:5 + 200].contiguous())
    assert torch.equal(shifted, big[5:205])
    assert torch.equal(_eval(eng, 0, rows[37:37 + 99], 78, 9), big[37:37 + 99])
    assert torch.equal(_eval(eng, 0, rows[n - 70:], 26, 9), big[n - 70:])
    # agent 1's network on the same rows is another network
    assert not torch.equal(eng.actor_logits(1, rows[:64].contiguous()), big[:64])


# ---- 3. against the closed loop --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def looped():
    """an engine with three tanh actors and a critic, and a batch of 20 steps collected with them (800 rows: 12 full tiles and a half)"""
    e = AR.engine(N, False)
    nets = [AR.torch_actor(300 + a) for a in range(3)]
    AR.set_actors(e, nets)
    e.set_critic(CR.make_critic(21), CR.VALUE_NORM)
    e.reset()
    batch = e.collect(20)
    yield e, nets, batch
    e.close()


def test_evaluate_actions_against_the_closed_loop(looped):
    import torch
    e, nets, b = looped
    T = b.n_steps
    logits, logp, ent = e.evaluate_actions(b.obs[:T], b.actions)
    assert logits.shape == (T, N, 3, 3) and logp.shape == ent.shape == (T, N, 3)
    dist = float((logits - b.logits).abs().max())
    print("evaluate_actions against the rollout kernel's logits on %d rows x 3 agents: max |difference| %.2e" % (T * N, dist))
    assert dist <= BAR
    for a in range(3):
        with torch.no_grad():
            ref = copy.deepcopy(nets[a]).double()(b.obs[:T, :, a].cpu().double())
        assert float((logits[:, :, a].cpu().double() - ref).abs().max()) <= BAR
    want_lp, want_ent = OR.action_log_probs(b.actions.cpu().numpy(), logits.cpu().numpy())
    assert OR.ulps(logp.cpu().numpy(), want_lp).max() <= 1 and OR.ulps(ent.cpu().numpy(), want_ent).max() <= 1
    again = e.evaluate_actions(b.obs[:T], b.actions)
    for x, y in zip((logits, logp, ent), again):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # a subset of the agents: the other columns of logits are zero, the asked ones the same bits
    l1, lp1, none = e.evaluate_actions(b.obs[:T], b.actions, agents=(1,), want_entropy=False)
    assert none is None and torch.equal(l1[:, :, 1], logits[:, :, 1]) and not l1[:, :, 0].any() and not l1[:, :, 2].any()
    assert torch.equal(lp1[:, :, 1], logp[:, :, 1])
    # the reference's own order of operations: both of the runner's evaluations go through evaluate_actions -- an unchanged actor has
    # ratio exactly 1
    for a in range(3):
        t = e.actor_update_terms(b, a, old_log_probs=logp)
        assert bool((t.ratio == 1.0).all()) and torch.equal(t.factor, t.ratio)
        s = t.summary()
        assert s["approx_kl"] == 0.0 and s["clip_frac"] == 0.0 and s["ratio_mean"] == 1.0 and s["ratio_min"] == s["ratio_max"] == 1.0
        adv = b.normalized_advantages()
        assert torch.equal(t.surr, adv)      # (min(1 A, 1 A) times a factor of one)
        assert abs(s["entropy"] - float(ent[:, :, a].double().mean())) <= 1e-12
    # against the closed loop's own log-probabilities the ratio is near one, not one
    t = e.actor_update_terms(b, 0)
    assert float((t.ratio - 1.0).abs().max()) <= 1e-3 and t.summary()["clip_frac"] == 0.0


# ---- 4. ppo_terms against the restatement --------------------------------------------------------------------------------------------------
def _ppo_inputs(T, n_envs, seed):
    """new, old [T, n, 3] per agent column built so (the other two columns NaN in the arrays the device gets), advantages, factor,
    entropy: lr from N(0, 0.15), every 7th element exactly 0, every 29th +-80; advantages of both signs, every 5th exactly 0"""
    rng = np.random.default_rng(seed)
    shape = (T, n_envs, 3)
    old = (-np.abs(rng.standard_normal(shape)) - 0.05).astype(np.float32)
    new = (old + (0.15 * rng.standard_normal(shape)).astype(np.float32)).astype(np.float32)
    flat_new, flat_old = new.reshape(-1, 3), old.reshape(-1, 3)
    k = np.arange(flat_new.shape[0])
    flat_new[k % 7 == 0] = flat_old[k % 7 == 0]
    far = k % 29 == 3
    flat_new[far] = flat_old[far] + np.where(k[far] % 2 == 0, np.float32(80.0), np.float32(-80.0))[:, None]
    adv = rng.standard_normal(shape[:2]).astype(np.float32)
    adv.reshape(-1)[k % 5 == 1] = 0.0
    factor = np.exp(0.1 * rng.standard_normal(shape[:2])).astype(np.float32)
    ent = rng.uniform(0.0, 1.0986, shape).astype(np.float32)
    return new, old, adv, factor, ent


def _column_only(x, agent):
    y = np.full(x.shape, POISON, dtype=np.float32)
    y[..., agent] = x[..., agent]
    return y


class _Tally:
    def __init__(self):
        self.n = self.differ = self.own = self.unsure = 0


def _check_ppo(e, tally, T, agent, clip, new, old, adv, factor, ent):
    """one ppo_terms call against the restatement, every check of the module docstring's item 4"""
    import torch
    dev = lambda x: None if x is None else torch.from_numpy(x).to(e.device)
    n_envs = e.n_envs
    new_d, old_d = _column_only(new, agent), _column_only(old, agent)
    ent_d = None if ent is None else _column_only(ent, agent)
    want = PR.terms(new, old, adv, agent, clip, factor)
    wide = PR.terms(new, old, adv, agent, clip, factor, np.longdouble)
    tally.own += int((PR.ulps(want["ratio"], wide["ratio"]) > 0).sum() + (PR.ulps(want["surr"], wide["surr"]) > 0).sum())
    got = e.ppo_terms(agent, dev(new_d), dev(old_d), dev(adv), clip, factor=dev(factor), entropy=dev(ent_d))
    ratio, surr, fout = (x.cpu().numpy() for x in (got.ratio, got.surr, got.factor))
    assert ratio.shape == surr.shape == fout.shape == (T, n_envs) and np.isfinite(ratio).all() and np.isfinite(surr).all()
    u_r, u_s = PR.ulps(ratio, want["ratio"]), PR.ulps(surr, want["surr"])
    assert u_r.max() <= 1 and u_s.max() <= 1, (T, agent, clip, int(u_r.max()), int(u_s.max()))
    tally.n += 2 * ratio.size
    tally.differ += int((u_r > 0).sum() + (u_s > 0).sum())
    # the factor: one fp32 product of the stored values
    f32 = np.ones_like(ratio) if factor is None else factor
    assert np.array_equal((f32 * ratio).view(np.uint32), fout.view(np.uint32))
    # the statistics, bit for bit from the device's own stored outputs; the clipped count up to the unsure elements
    stats = got.stats.cpu().numpy()
    ref = PR.stats(surr, ratio, want["lr"], None if ent is None else ent[..., agent], want["clipped"])
    for q in (0, 1, 2, 3, 5, 6, 7):
        assert stats[q] == ref[q] and np.signbit(stats[q]) == np.signbit(ref[q]), (T, agent, clip, q, stats[q], ref[q])
    unsure = int(want["unsure"].sum())
    assert abs(stats[4] - ref[4]) <= unsure, (stats[4], ref[4], unsure)
    tally.unsure += unsure
    # without surr and statistics' inputs the rest is the same bits
    bare = e.ppo_terms(agent, dev(new_d), dev(old_d), dev(adv), clip, factor=dev(factor), want_surr=False)
    assert bare.surr is None and torch.equal(bare.ratio, got.ratio) and torch.equal(bare.factor, got.factor)
    sb = bare.stats.cpu().numpy()
    assert sb[3] == 0.0 and all(sb[q] == stats[q] for q in (0, 1, 2, 4, 5, 6, 7))
    return got


def test_ppo_terms_against_the_restatement(eng):
    import torch
    T = 37
    tally = _Tally()
    for agent in range(3):
        new, old, adv, factor, ent = _ppo_inputs(T, N, 50 + agent)
        for clip in (0.2, 0.0):
            for with_factor in (True, False):
                for with_ent in (True, False):
                    got = _check_ppo(eng, tally, T, agent, clip, new, old, adv, factor if with_factor else None, ent if with_ent else None)
            if clip == 0.0:      # every element with r != 1 counts as clipped
                assert got.stats[4].item() == float((new[..., agent] != old[..., agent]).sum())
        # in place, and without statistics: the raw call with factor_out = factor and stats = NULL
        dev = lambda x: torch.from_numpy(x).to(eng.device)
        nd, od, ad, fd = dev(_column_only(new, agent)), dev(_column_only(old, agent)), dev(adv), dev(factor)
        ratio = torch.empty((T, N), device=eng.device)
        p = lambda x: x.data_ptr()
        eng._call(eng.lib.sdc_ppo_terms, T, agent, p(nd), p(od), None, p(ad), p(fd), 0.2, p(ratio), None, p(fd), None, eng._stream(),
                  refuses=True)
        assert np.array_equal((factor * ratio.cpu().numpy()).view(np.uint32), fd.cpu().numpy().view(np.uint32))
        assert torch.equal(ratio, got.ratio)
    print("sdc_ppo_terms at T = %d, N = %d: %d results; different from the restatement (all by 1 ulp): %d; fp64 against long double in the "
          "restatement itself: %d; unsure of their clip edge: %d" % (T, N, tally.n, tally.differ, tally.own, tally.unsure))
    assert tally.own * 1000 <= tally.n, "choose other seeds: fp64 itself moves more than 1 result in 1000 on these inputs"
    assert tally.differ * 1000 <= tally.n and tally.unsure <= AR.UNSURE_CAP * tally.n


def test_ppo_terms_sizes_around_a_workgroup_and_above_the_stage_one_cap():
    """T N of 1, 255, 256, 257 and 256 * 1024 + 77 (an engine of one env: T N = T): the grid-stride loop, both halving trees with empty
    lanes, and the second stage's loop"""
    one = AR.engine(1, False)
    try:
        tally = _Tally()
        for i, T in enumerate((1, 255, 256, 257, L.PPO_BLOCK * L.PPO_MAX_BLOCKS + 77)):
            new, old, adv, factor, ent = _ppo_inputs(T, 1, 70 + i)
            _check_ppo(one, tally, T, i % 3, 0.2, new, old, adv, factor, ent)
        assert tally.differ * 1000 <= max(tally.n, 1000) and tally.own * 1000 <= max(tally.n, 1000)
        assert tally.unsure <= max(AR.UNSURE_CAP * tally.n, 1)
    finally:
        one.close()


# ---- 5. the HAPPO chain --------------------------------------------------------------------------------------------------------------------
def _perturbed(net, seed):
    import torch
    m = copy.deepcopy(net)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn(p.shape, generator=g))
    return m


def test_happo_chain_vector_env_and_deepcopy(looped):
    import torch
    from tests.test_gpu_actor_stats import _vec
    e, nets, b = looped
    T = 8
    from dc_rl_amd.engine import OnPolicyBatch
    fields = {k: getattr(b, k) for k in b.FIELDS}      # (the first 8 steps; the moments stay the whole batch's: constants here)
    fields.update(obs=b.obs[:T + 1], actions=b.actions[:T], action_log_probs=b.action_log_probs[:T], advantages=b.advantages[:T])
    small = OnPolicyBatch(**fields)
    assert small.n_steps == T
    obs, acts = small.obs[:T], small.actions
    adv = small.normalized_advantages()
    v = _vec(N)
    try:
        v.reset()
        factor, factor_np = None, None
        current = list(nets)
        for a in (2, 0, 1):
            _, old, _ = e.evaluate_actions(obs, acts, agents=(a,))
            current[a] = _perturbed(nets[a], 700 + a)
            e.set_actor(a, dict(current[a].state_dict(), activation="tanh"))
            t = e.actor_update_terms(small, a, 0.2, factor=factor, old_log_probs=old)
            # the runner's loop restated: new = evaluate after the update, factor = factor * exp(new - old)
            _, new, ent = e.evaluate_actions(obs, acts, agents=(a,))
            w = PR.terms(new.cpu().numpy(), old.cpu().numpy(), adv.cpu().numpy(), a, 0.2, factor_np)
            for name, got in (("ratio", t.ratio), ("surr", t.surr), ("factor_out", t.factor)):
                assert np.array_equal(got.cpu().numpy().view(np.uint32), w[name].view(np.uint32)), (a, name)
            ref = PR.stats(w["surr"], w["ratio"], w["lr"], ent.cpu().numpy()[..., a], w["clipped"])
            assert np.array_equal(t.stats.cpu().numpy(), ref) and not w["unsure"].any()
            assert float((t.ratio - 1.0).abs().max()) > 1e-3      # (the update moved the actor)
            factor, factor_np = t.factor, w["factor_out"]
        # the vector env's delegates, with the same actors, give the same tensors
        for a in range(3):
            v.set_actor(a, current[a].state_dict())
        dev = v.engine.device
        lg, lp, en = e.evaluate_actions(obs, acts)
        for x, y in zip((lg, lp, en), v.evaluate_actions(obs.to(dev), acts.to(dev))):
            assert torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32))
        assert torch.equal(v.actor_logits(2, obs.to(dev)).cpu(), lg[:, :, 2].cpu())
        mine = e.ppo_terms(1, lp, small.action_log_probs, adv, 0.1, factor=factor, entropy=en)
        theirs = v.ppo_terms(1, lp.to(dev), small.action_log_probs.to(dev), adv.to(dev), 0.1, factor=factor.to(dev), entropy=en.to(dev))
        for name in ("ratio", "surr", "factor", "stats"):
            assert torch.equal(getattr(mine, name).cpu(), getattr(theirs, name).cpu()), name
        # copy.deepcopy carries the actors: the copy's engine evaluates to the same bits
        c = copy.deepcopy(v)
        try:
            for x, y in zip((lg, lp, en), c.evaluate_actions(obs.to(dev), acts.to(dev))):
                assert torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32))
        finally:
            c.close()
    finally:
        v.close()
        AR.set_actors(e, nets)


# ---- 6. refusal wiring ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_reaches_python_and_nothing_is_launched(looped):
    import torch
    e, nets, b = looped
    dev, T = e.device, 3
    obs = torch.zeros((T, N, 3, 26), device=dev)
    out = _poisoned(torch, T * N * 9, dev)
    p = lambda x: x.data_ptr()
    ev = lambda **kw: e._call(e.lib.sdc_actor_evaluate, kw.get("agent", 0), kw.get("obs", p(obs)), kw.get("stride", 78), kw.get("rows", T * N),
                              kw.get("out", p(out)), kw.get("ls", 9), e._stream(), refuses=True)
    refused(e, "sdc_actor_evaluate: agent_slot = 3 outside \\[0, 2\\]", lambda: ev(agent=3))
    refused(e, "sdc_actor_evaluate: n_rows = 0 must be positive", lambda: ev(rows=0))
    refused(e, "sdc_actor_evaluate: null array \\(obs and logits are required\\)", lambda: ev(obs=None))
    refused(e, "sdc_actor_evaluate: null array \\(obs and logits are required\\)", lambda: ev(out=None))
    refused(e, "sdc_actor_evaluate: obs / logits not dword-aligned", lambda: ev(obs=p(obs) + 2))
    refused(e, "sdc_actor_evaluate: row_stride = 25 below a row's 26 floats", lambda: ev(stride=25))
    refused(e, "sdc_actor_evaluate: logits_stride = 2 below a row's 3 floats", lambda: ev(ls=2))
    lp = torch.zeros((T, N, 3), device=dev)
    adv = torch.zeros((T, N), device=dev)
    ratio = _poisoned(torch, T * N, dev).view(T, N)
    stats = torch.zeros(9, dtype=torch.float64, device=dev)
    pp = lambda **kw: e._call(e.lib.sdc_ppo_terms, kw.get("T", T), kw.get("agent", 0), kw.get("new", p(lp)), p(lp), None, kw.get("adv", p(adv)),
                              None, kw.get("clip", 0.2), kw.get("ratio", p(ratio)), kw.get("surr"), None, kw.get("stats"), e._stream(),
                              refuses=True)
    refused(e, "sdc_ppo_terms: n_steps = 0 must be positive", lambda: pp(T=0))
    refused(e, "sdc_ppo_terms: agent = -1 outside \\[0, 2\\]", lambda: pp(agent=-1))
    refused(e, "sdc_ppo_terms: null array \\(new_log_probs, old_log_probs, advantages and ratio are required\\)", lambda: pp(new=None))
    refused(e, "sdc_ppo_terms: null array", lambda: pp(adv=None))
    refused(e, "sdc_ppo_terms: null array", lambda: pp(ratio=None))
    refused(e, "sdc_ppo_terms: new_log_probs / old_log_probs / entropy / advantages / factor / ratio / surr / factor_out not dword-aligned",
            lambda: pp(surr=p(adv) + 1))
    refused(e, "sdc_ppo_terms: stats not 8-byte aligned", lambda: pp(stats=p(stats) + 4))
    for bad in (1.0, -0.1, float("nan"), float("inf")):
        refused(e, "sdc_ppo_terms: clip_param = .* outside \\[0, 1\\)", lambda: e.ppo_terms(0, lp, lp, adv, bad))
    # the Python side's own checks, in its words
    refused(e, "actor_logits: agent = 3 must be 0 \\(ls\\), 1 \\(dc\\) or 2 \\(bat\\)", lambda: e.actor_logits(3, obs))
    refused(e, "actor_logits: obs must be a contiguous float32 CUDA tensor of shape \\(\\.\\.\\., 26\\) or \\(\\.\\.\\., 3, 26\\)",
            lambda: e.actor_logits(0, obs[..., :25]))
    refused(e, "actor_logits: obs must be", lambda: e.actor_logits(0, obs.cpu()))
    refused(e, "actor_logits: obs must be", lambda: e.actor_logits(0, obs[:0]))
    refused(e, "actor_logits: per_agent asks for", lambda: e.actor_logits(0, obs[:, :, 0].contiguous(), per_agent=True))
    refused(e, "evaluate_actions: obs must be .* \\(T, n_envs, 3, 26\\)", lambda: e.evaluate_actions(obs[:2], b.actions[:T]))
    refused(e, "evaluate_actions: actions must be", lambda: e.evaluate_actions(obs, b.actions[:T].long()))
    refused(e, "evaluate_actions: agents = \\(0, 0\\) must name", lambda: e.evaluate_actions(obs, b.actions[:T], agents=(0, 0)))
    refused(e, "ppo_terms: old_log_probs must be", lambda: e.ppo_terms(0, lp, lp[:2], adv))
    refused(e, "ppo_terms: advantages must be .* \\(T, n_envs\\)", lambda: e.ppo_terms(0, lp, lp, lp))
    refused(e, "ppo_terms: factor must be", lambda: e.ppo_terms(0, lp, lp, adv, factor=lp))
    refused(e, "ppo_terms: entropy must be", lambda: e.ppo_terms(0, lp, lp, adv, entropy=adv))
    refused(e, "ppo_terms: agent = 'a' must be", lambda: e.ppo_terms("a", lp, lp, adv))
    # nothing was launched: the outputs the refused calls were given are still poison
    torch.cuda.synchronize(dev)
    assert _is_poison(out) and _is_poison(ratio)
    # an engine without an actor for the slot
    bare = AR.engine(N, False)
    try:
        bare.set_actor(0, dict(nets[0].state_dict(), activation="tanh"))
        assert bare.actor_logits(0, obs).shape == (T, N, 3)
        with pytest.raises(ValueError, match="sdc_actor_evaluate: no actor is set for agent_slot 2 \\(sdc_set_actor first\\)"):
            bare.actor_logits(2, obs)
        with pytest.raises(ValueError, match="sdc_actor_evaluate: no actor is set for agent_slot 1"):
            bare.evaluate_actions(obs, b.actions[:T])
    finally:
        bare.close()
