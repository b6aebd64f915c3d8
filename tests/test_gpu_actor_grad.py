"""sdc_actor_backward and sdc_ppo_dlogp on the device (include/sustaindc_hip.h THE ACTORS' GRADIENT) against the NumPy fp64 restatement
(tests/actor_grad_ref.py), under the measure max|delta| / max|g| per parameter tensor, the worst tensor against the bar
8 x (torch fp32 CPU autograd's worst distance from the restatement on the same inputs) -- the reference arithmetic, not the code under
test; the margin: the forward sits 2-3x from torch fp32's own distance (hardware exp2 / rcp / rsq, one-pass moments), the backward passes
that through two more LayerNorms and sums rows in another order.  DESIGN.md section 4.28 records both columns per configuration.

1. the gradients of the four configurations at row strides 26 and 78, action strides 1 and 3, row counts around a tile, around a
   workgroup and SDC_ACTOR_GRAD_MAX_BLOCKS * 64 + 17 (the grid's second pass, the prefetch across it, a last tile of one row); every
   call with NaN observations, garbage actions and NaN coefficients behind row n_rows and poison behind element 6390 of grads; the
   rows come from a pool of 200 distinct rows per configuration whose relu pre-activations keep 1e-5 from zero (asserted: a unit that
   straddles zero legitimately flips between fp32 and fp64);
2. bitwise: the same call twice, in place against gathered, doubled coefficients, zero coefficients, grad_sq from the device's own
   grads in the header's order, the feature LayerNorm off;
3. edges: actions outside 0 .. 2, a dead relu layer;
4. ppo_dlogp against the restatement to one ulp, bit-equal where the ratio is exactly 1 or the advantage exactly 0;
5. the loop closed on a collected batch: actor_grads against the restatement, three SGD steps that lower the loss and track a torch
   fp64 run, the vector env's delegates, every refusal as ValueError with the library's text."""
import copy

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import actor_grad_ref as GR
from tests import actor_ref as AR
from tests import critic_ref as CR
from tests import onpolicy_ref as OR
from tests import ppo_ref as PR
from tests.plan_util import refused

pytestmark = pytest.mark.gpu

N = 40
MARGIN = 8.0
POOL = 200
LARGE = L.ACTOR_GRAD_MAX_BLOCKS * 64 + 17
COUNTS = [1, 15, 16, 17, 63, 64, 65, 67, LARGE]
POOL_SEED = {"tanh_fn1": 900, "tanh_fn0": 901, "relu_fn1": 912, "relu_fn0": 913}      # (relu: the margin below holds; checked on the CPU)
NAN32 = np.array([OR.NAN_BITS], dtype=np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def eng():
    e = AR.engine(N, False)
    yield e
    e.close()


def pool(activation, feature_norm):
    """200 distinct observation rows of the fixture's kind"""
    rng = np.random.default_rng(POOL_SEED[GR.cfg_name(activation, feature_norm)])
    x = rng.standard_normal((POOL, 26)).astype(np.float32)
    x[1::3, 14:] = 0.0
    x[2::3, 13:] = 0.0
    return x


def inputs(activation, feature_norm, rows, seed):
    """rows of the pool (tiled past 200) with fresh actions and coefficients: -> x [R, 26], actions [R], dlogp [R], dent"""
    rng = np.random.default_rng(seed)
    x = pool(activation, feature_norm)[np.arange(rows) % POOL]
    actions = rng.integers(0, 3, size=rows).astype(np.int32)
    coef = (rng.standard_normal(rows) / rows).astype(np.float32)
    coef[3::7] = 0.0
    return x, actions, coef, -0.01 / rows


def backward(e, agent, x, actions, coef, dent, stride=26, astride=1, want_sq=True):
    """sdc_actor_backward of the rows placed `stride` floats apart (at the agent's place of [R][3][26] when 78), the actions `astride`
    apart (the agent's column of [R][3] when 3), in buffers whose every other entry -- and three more rows behind row R -- is NaN /
    garbage, into grads with 7 poisoned floats behind it -> (grads fp32 [6391], grad_sq float or None)"""
    import torch
    R, extra = x.shape[0], 3
    off = 26 * agent if stride == 78 else 0
    aoff = agent if astride == 3 else 0
    obs = np.full((R + extra, stride), NAN32, dtype=np.float32)
    obs[:R, off:off + 26] = x
    act = np.full((R + extra, astride), 0x7FFFFFF1, dtype=np.int32)
    act[:R, aoff] = actions
    cf = np.full(R + extra, NAN32, dtype=np.float32)
    cf[:R] = coef
    dev = lambda a: torch.from_numpy(a).to(e.device)
    obs_d, act_d, cf_d = dev(obs), dev(act), dev(cf)
    out = torch.full((L.ACTOR_N_PARAMS + 7,), OR.NAN_BITS, dtype=torch.int32, device=e.device).view(torch.float32)
    sq = torch.full((1,), -1.0, dtype=torch.float64, device=e.device) if want_sq else None
    e._behind_torch_stream()
    e._call(e.lib.sdc_actor_backward, agent, obs_d.data_ptr() + 4 * off, stride, R, act_d.data_ptr() + 4 * aoff, astride, cf_d.data_ptr(),
            float(dent), out.data_ptr(), None if sq is None else sq.data_ptr(), e._stream(), refuses=True)
    got = out.cpu().numpy()
    assert (got[L.ACTOR_N_PARAMS:].view(np.uint32) == np.uint32(OR.NAN_BITS)).all()      # (the poison behind element 6390)
    g = got[:L.ACTOR_N_PARAMS].copy()
    assert np.isfinite(g).all(), (R, stride, astride)
    return g, (None if sq is None else float(sq.cpu()[0]))


def bar_of(sd, activation, x, actions, coef, dent, want):
    """torch fp32 CPU autograd's worst distance from the restatement `want` on these inputs"""
    import torch
    t32 = GR.torch_grads(GR.torch_net(sd, activation, torch.float32), x, actions, coef, dent)
    return max(GR.distance(t32, want).values())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the gradients --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,feature_norm", GR.CONFIGS)
def test_gradients_against_the_restatement(eng, activation, feature_norm):
    c = GR.case(activation, feature_norm)
    name = GR.cfg_name(activation, feature_norm)
    agent = GR.CONFIGS.index((activation, feature_norm)) % 3
    eng.set_actor(agent, dict(c["sd"], activation=activation))
    worst = (0.0, 0.0, None)
    for rows in COUNTS:
        x, actions, coef, dent = inputs(activation, feature_norm, rows, 40 + rows)
        want = GR.backward(c["sd"], x, actions, coef, dent, activation)
        if activation == "relu":
            assert GR.relu_margin(want) > 1e-5, (name, rows, GR.relu_margin(want))
        scale = bar_of(c["sd"], activation, x, actions, coef, dent, want)
        for stride, astride in ((26, 1), (78, 3)):
            g, sq = backward(eng, agent, x, actions, coef, dent, stride, astride)
            dist = GR.distance(GR.split(g), want)
            d = max(dist.values())
            print("%s %5d rows strides %2d/%d: device %.2e (%s), torch fp32 %.2e, ratio %.1f" % (
                name, rows, stride, astride, d, max(dist, key=dist.get), scale, d / scale))
            if d / scale > worst[0] / max(worst[1], 1e-300) or worst[2] is None:
                worst = (d, scale, rows)
            assert d <= MARGIN * scale, (name, rows, stride, astride, dist, scale)
            assert sq == GR.grad_sq(g), (name, rows, sq, GR.grad_sq(g))
            if not feature_norm:
                assert not g[:52].any() and not np.signbit(g[:52]).any()      # (exact zeros)
    print("%s: worst device %.2e against torch fp32 %.2e at %d rows" % ((name,) + worst))


# ---- 2. bitwise ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,feature_norm,rows", [("tanh", True, 67), ("relu", False, 150), ("tanh", False, LARGE)])
def test_bitwise_properties(eng, activation, feature_norm, rows):
    c = GR.case(activation, feature_norm)
    eng.set_actor(1, dict(c["sd"], activation=activation))
    x, actions, coef, dent = inputs(activation, feature_norm, rows, 7)
    g, sq = backward(eng, 1, x, actions, coef, dent)
    again, sq2 = backward(eng, 1, x, actions, coef, dent)
    assert np.array_equal(bits(g), bits(again)) and sq == sq2                                     # the same call twice
    placed, sq3 = backward(eng, 1, x, actions, coef, dent, 78, 3)
    assert np.array_equal(bits(g), bits(placed)) and sq == sq3                                    # in place against gathered
    twice, sq4 = backward(eng, 1, x, actions, coef * np.float32(2.0), 2.0 * dent)
    assert np.array_equal(bits(twice), bits(g * np.float32(2.0)))                                 # doubled exactly
    zero, sq0 = backward(eng, 1, x, actions, np.zeros_like(coef), 0.0)
    assert not zero.any() and sq0 == 0.0                                                          # all-zero coefficients
    assert sq == GR.grad_sq(g) and sq4 == GR.grad_sq(twice)                                       # grad_sq from the device's own grads
    bare, none = backward(eng, 1, x, actions, coef, dent, want_sq=False)
    assert none is None and np.array_equal(bits(g), bits(bare))
    if not feature_norm:
        assert not g[:52].any()


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------------
def test_actions_outside_the_range_are_an_all_zero_one_hot(eng):
    activation, feature_norm = "tanh", True
    c = GR.case(activation, feature_norm)
    eng.set_actor(0, dict(c["sd"], activation=activation))
    x, actions, coef, dent = inputs(activation, feature_norm, 67, 11)
    actions[::4] = np.array([-1, 3, 2 ** 31 - 1, -2 ** 31, 7], dtype=np.int64).astype(np.int32)[np.arange(len(actions[::4])) % 5]
    want = GR.backward(c["sd"], x, actions, coef, dent, activation)
    scale = bar_of(c["sd"], activation, x, actions, coef, dent, want)
    for stride, astride in ((26, 1), (78, 3)):
        g, _ = backward(eng, 0, x, actions, coef, dent, stride, astride)
        d = max(GR.distance(GR.split(g), want).values())
        print("actions outside 0..2: device %.2e, torch fp32 %.2e" % (d, scale))
        assert d <= MARGIN * scale


@pytest.mark.parametrize("feature_norm", [True, False])
def test_a_dead_relu_layer(eng, feature_norm):
    c = GR.case("relu", feature_norm)
    sd = {k: v.copy() for k, v in c["sd"].items()}
    sd[GR.KEYS["b1"]][:] = -1000.0
    eng.set_actor(2, dict(sd, activation="relu"))
    x, actions, coef, dent = inputs("relu", feature_norm, 67, 13)
    want = GR.backward(sd, x, actions, coef, dent, "relu")
    assert (want["z1"] < -100.0).all() and np.abs(want["z2"]).min() > 1e-5
    scale = bar_of(sd, "relu", x, actions, coef, dent, want)
    g, sq = backward(eng, 2, x, actions, coef, dent, 78, 3)
    got = GR.split(g)
    for k in ("w1", "b1", "ln0_gamma", "ln0_beta"):
        assert not got[k].any() and not want[k].any(), k
    d = max(GR.distance(got, want).values())
    print("dead relu layer fn%d: device %.2e, torch fp32 %.2e" % (feature_norm, d, scale))
    assert d <= MARGIN * scale and np.isfinite(g).all() and sq == GR.grad_sq(g)


# ---- 4. ppo_dlogp ------------------------------------------------------------------------------------------------------------------------------
def test_ppo_dlogp_against_the_restatement(eng):
    import torch
    from tests.test_gpu_actor_eval import _column_only, _ppo_inputs
    T = 37
    dev = lambda a: None if a is None else torch.from_numpy(a).to(eng.device)
    checked = differ = 0
    for agent in range(3):
        new, old, adv, factor, _ = _ppo_inputs(T, N, 60 + agent)
        new_d, old_d = _column_only(new, agent), _column_only(old, agent)      # (the other two columns NaN)
        for clip in (0.2, 0.0):
            for f in (factor, None):
                for scale in (None, 0.37):
                    want, r, is_open, _ = GR.dlogp(new, old, adv, agent, clip, f, scale)
                    unsure = PR.terms(new, old, adv, agent, clip, f)["unsure"]
                    got = eng.ppo_dlogp(agent, dev(new_d), dev(old_d), dev(adv), clip, factor=dev(f), scale=scale).cpu().numpy()
                    assert got.shape == (T, N) and got.dtype == np.float32 and np.isfinite(got).all()
                    u = PR.ulps(got, want)
                    assert u[~unsure].max() <= 1, (agent, clip, scale, int(u[~unsure].max()))
                    exact = (r == 1.0) | (adv == 0.0)
                    assert exact.sum() > 100 and np.array_equal(bits(got[exact]), bits(want[exact]))
                    assert (got[(adv == 0.0)] == 0.0).all() and (np.abs(np.log(r)) > 70).sum() > 10
                    checked += int((~unsure).sum())
                    differ += int((u[~unsure] > 0).sum())
    print("ppo_dlogp: %d elements, %d one ulp from the restatement" % (checked, differ))


# ---- 5. the loop closed --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def looped():
    """an engine with three tanh actors and a critic, and a batch of 20 steps collected with them"""
    e = AR.engine(N, False)
    nets = [AR.torch_actor(300 + a) for a in range(3)]
    AR.set_actors(e, nets)
    e.set_critic(CR.make_critic(21), CR.VALUE_NORM)
    e.reset()
    batch = e.collect(20)
    yield e, nets, batch
    e.close()


def _torch_loss(net, x, actions, old, adv, clip, coef_ent):
    """happo.py's policy_loss - entropy_coef * dist_entropy in the module's dtype (every active mask one, factor one)"""
    import torch
    dt = next(net.parameters()).dtype
    logp_all = torch.log_softmax(net(x.to(dt)), -1)
    logp = logp_all.gather(-1, actions.long()[:, None])[:, 0]
    ratio = torch.exp(logp - old.to(dt))
    A = adv.to(dt)
    policy = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * A).mean()
    entropy = -(logp_all.exp() * logp_all).sum(-1).mean()
    return policy - coef_ent * entropy


def test_actor_grads_close_the_loop(looped):
    import torch
    from tests.test_gpu_actor_stats import _vec
    e, nets, b = looped
    T, a, clip, coef_ent, lr = b.n_steps, 1, 0.2, 0.01, 0.02
    try:
        grads, terms = e.actor_grads(b, a, clip, coef_ent)
        assert grads.flat.shape == (L.ACTOR_N_PARAMS,) and grads.sq_norm.dim() == 0
        # against the restatement fed the batch's own tensors (the device's log-probabilities of its own forward are the ratio's)
        x = b.obs[:T, :, a].reshape(T * N, 26).cpu().numpy()
        acts = b.actions[..., a].reshape(-1).cpu().numpy()
        _, logp, _ = e.evaluate_actions(b.obs[:T], b.actions, agents=(a,))
        adv = b.normalized_advantages()
        d32, r, _, _ = GR.dlogp(logp.cpu().numpy(), b.action_log_probs.cpu().numpy(), adv.cpu().numpy(), a, clip)
        assert np.minimum(np.abs(r - 0.8), np.abs(r - 1.2)).min() > 1e-6
        dlogp_dev = e.ppo_dlogp(a, logp, b.action_log_probs, adv, clip).cpu().numpy()
        assert PR.ulps(dlogp_dev, d32).max() <= 1
        dlogp_dev = dlogp_dev.reshape(-1)
        sd = {k: v.detach().numpy() for k, v in nets[a].state_dict().items()}
        dent = -coef_ent / (T * N)
        want = GR.backward(sd, x, acts, dlogp_dev, dent, "tanh")
        scale = bar_of(sd, "tanh", x, acts, dlogp_dev, dent, want)
        g = grads.flat.cpu().numpy()
        d = max(GR.distance(GR.split(g), want).values())
        print("actor_grads on %d rows: device %.2e, torch fp32 %.2e" % (T * N, d, scale))
        assert d <= MARGIN * scale
        assert float(grads.sq_norm.cpu()) == GR.grad_sq(g) and abs(float(grads.norm().cpu()) - np.sqrt(GR.grad_sq(g))) <= 1e-15
        named = grads.named()
        assert list(named) == list(GR.FIELDS) and all(tuple(named[k].shape) == GR.SHAPES[k] for k in GR.FIELDS)
        assert set(grads.state_dict()) == set(nets[a].state_dict())
        # the vector env's delegates return the same tensors
        v = _vec(N)
        try:
            v.reset()
            v.set_actor(a, nets[a].state_dict())
            dv = v.engine.device
            theirs = v.actor_backward(a, b.obs[:T].to(dv), b.actions.to(dv), torch.from_numpy(dlogp_dev).view(T, N).to(dv), dent)
            assert torch.equal(theirs.flat.cpu(), grads.flat.cpu()) and torch.equal(theirs.sq_norm.cpu(), grads.sq_norm.cpu())
            assert torch.equal(v.ppo_dlogp(a, logp.to(dv), b.action_log_probs.to(dv), adv.to(dv), clip).cpu().view(-1),
                               torch.from_numpy(dlogp_dev))
        finally:
            v.close()
        # clip_: torch's clip_grad_norm_ rule
        before = grads.flat.clone()
        total = grads.clip_(0.5 * float(grads.norm()))
        assert float(total) == float(grads.norm()) and torch.allclose(grads.flat, before * 0.5, rtol=1e-5, atol=0.0)
        untouched = e.actor_backward(a, b.obs[:T], b.actions, torch.from_numpy(dlogp_dev).view(T, N).to(e.device), dent)
        assert torch.equal(untouched.flat, before)
        assert float(untouched.clip_(1e9)) == float(untouched.norm()) and torch.equal(untouched.flat, before)
        # three SGD steps through a plain torch module and set_actor; a torch fp64 run of the same three steps beside them
        mod = copy.deepcopy(nets[a])
        ref = copy.deepcopy(nets[a]).double()
        opt, opt_ref = torch.optim.SGD(mod.parameters(), lr=lr), torch.optim.SGD(ref.parameters(), lr=lr)
        xt, at = torch.from_numpy(x), torch.from_numpy(acts)
        old, advc = b.action_log_probs[..., a].reshape(-1).cpu(), adv.reshape(-1).cpu()
        losses, losses_ref = [], []
        for step in range(4):
            gr, tm = e.actor_grads(b, a, clip, coef_ent)
            s = tm.summary()
            losses.append(s["policy_loss"] - coef_ent * s["entropy"])
            opt_ref.zero_grad()
            loss_ref = _torch_loss(ref, xt, at, old, advc, clip, coef_ent)
            losses_ref.append(float(loss_ref.detach()))
            if step == 3:
                break
            loss_ref.backward()
            opt_ref.step()
            gr.assign_to(mod)
            assert all(p.grad is not None and p.grad.shape == p.shape for p in mod.parameters())
            opt.step()
            e.set_actor(a, dict(mod.state_dict(), activation="tanh"))
        gap = max(abs(x1 - x2) for x1, x2 in zip(losses, losses_ref))
        print("loss over three SGD steps: device %s, torch fp64 %s, gap %.2e" % (losses, losses_ref, gap))
        assert all(losses[i + 1] < losses[i] for i in range(3)), losses
        assert gap <= 1e-4, gap      # (the logits agree to 2e-4, the project's bar for these actors; the loss averages 800 rows of them)
    finally:
        AR.set_actors(e, nets)


def test_every_refusal_reaches_python_and_nothing_is_launched(looped):
    import torch
    e, nets, b = looped
    dev, T = e.device, 3
    obs = torch.zeros((T, N, 3, 26), device=dev)
    acts = torch.zeros((T, N, 3), dtype=torch.int32, device=dev)
    cf = torch.zeros((T, N), device=dev)
    out = torch.full((L.ACTOR_N_PARAMS,), OR.NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    sq = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    p = lambda x: x.data_ptr()
    bw = lambda **kw: e._call(e.lib.sdc_actor_backward, kw.get("agent", 0), kw.get("obs", p(obs)), kw.get("stride", 78), kw.get("rows", T * N),
                              kw.get("acts", p(acts)), kw.get("astride", 3), kw.get("cf", p(cf)), kw.get("dent", 0.0), kw.get("out", p(out)),
                              kw.get("sq", p(sq)), e._stream(), refuses=True)
    refused(e, "sdc_actor_backward: agent_slot = 3 outside \\[0, 2\\]", lambda: bw(agent=3))
    refused(e, "sdc_actor_backward: n_rows = 0 must be positive", lambda: bw(rows=0))
    for name in ("obs", "acts", "cf", "out"):
        refused(e, "sdc_actor_backward: null array \\(obs, actions, dlogp and grads are required\\)", lambda: bw(**{name: None}))
    refused(e, "sdc_actor_backward: obs / actions / dlogp / grads not dword-aligned", lambda: bw(cf=p(cf) + 2))
    refused(e, "sdc_actor_backward: grad_sq not 8-byte aligned", lambda: bw(sq=p(sq) + 4))
    refused(e, "sdc_actor_backward: row_stride = 25 below a row's 26 floats", lambda: bw(stride=25))
    refused(e, "sdc_actor_backward: action_stride = 0 must be positive", lambda: bw(astride=0))
    for bad in (float("nan"), float("inf")):
        refused(e, "sdc_actor_backward: dent = .* is not finite", lambda: e.actor_backward(0, obs, acts, cf, dent=bad))
    lp = torch.zeros((T, N, 3), device=dev)
    dl = torch.full((T * N,), OR.NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    dp = lambda **kw: e._call(e.lib.sdc_ppo_dlogp, kw.get("T", T), kw.get("agent", 0), kw.get("new", p(lp)), p(lp), kw.get("adv", p(cf)),
                              kw.get("factor"), kw.get("clip", 0.2), kw.get("scale", 1.0), kw.get("out", p(dl)), e._stream(), refuses=True)
    refused(e, "sdc_ppo_dlogp: n_steps = 0 must be positive", lambda: dp(T=0))
    refused(e, "sdc_ppo_dlogp: agent = -1 outside \\[0, 2\\]", lambda: dp(agent=-1))
    refused(e, "sdc_ppo_dlogp: null array \\(new_log_probs, old_log_probs, advantages and dlogp are required\\)", lambda: dp(out=None))
    refused(e, "sdc_ppo_dlogp: null array", lambda: dp(new=None))
    refused(e, "sdc_ppo_dlogp: new_log_probs / old_log_probs / advantages / factor / dlogp not dword-aligned", lambda: dp(factor=p(cf) + 1))
    refused(e, "sdc_ppo_dlogp: clip_param = .* outside \\[0, 1\\)", lambda: dp(clip=1.0))
    for bad in (float("nan"), float("inf")):
        refused(e, "sdc_ppo_dlogp: scale = .* is not finite", lambda: e.ppo_dlogp(0, lp, lp, cf, scale=bad))
    # the Python side's own checks, in its words
    refused(e, "actor_backward: agent = 3 must be 0 \\(ls\\), 1 \\(dc\\) or 2 \\(bat\\)", lambda: e.actor_backward(3, obs, acts, cf))
    refused(e, "actor_backward: obs must be a contiguous float32 CUDA tensor", lambda: e.actor_backward(0, obs.cpu(), acts, cf))
    refused(e, "actor_backward: actions must be a contiguous int32 CUDA tensor of shape \\(3, 40\\) or \\(3, 40, 3\\)",
            lambda: e.actor_backward(0, obs, acts.long(), cf))
    refused(e, "actor_backward: dlogp must be", lambda: e.actor_backward(0, obs, acts, cf[:2]))
    refused(e, "actor_backward: dent = 'x' must be a number", lambda: e.actor_backward(0, obs, acts, cf, dent="x"))
    refused(e, "ppo_dlogp: advantages must be .* \\(T, n_envs\\)", lambda: e.ppo_dlogp(0, lp, lp, lp))
    refused(e, "ppo_dlogp: factor must be", lambda: e.ppo_dlogp(0, lp, lp, cf, factor=lp))
    refused(e, "actor_grads: agent = 5 must be", lambda: e.actor_grads(b, 5))
    # before set_actor: the library's text
    fresh = AR.engine(N, False)
    try:
        with pytest.raises(ValueError, match="sdc_actor_backward: no actor is set for agent_slot 1 \\(sdc_set_actor first\\)"):
            fresh.actor_backward(1, obs.to(fresh.device), acts.to(fresh.device), cf.to(fresh.device))
    finally:
        fresh.close()
    torch.cuda.synchronize(dev)
    assert bool((out.view(torch.int32) == OR.NAN_BITS).all()) and bool((dl.view(torch.int32) == OR.NAN_BITS).all()) and float(sq[0]) == -1.0
