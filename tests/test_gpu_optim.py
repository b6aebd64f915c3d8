"""sdc_actor_adam_step, sdc_critic_adam_step, sdc_get_*, sdc_*_optim and sdc_set_critic_norm on the device (include/sustaindc_hip.h THE
OPTIMISER STEP) against the NumPy restatement tests/optim_ref.py.  Shapes: 37 steps x 40 envs of stored rows, collect(20) at 40 envs.

1. after 1, 2, 3 and 10 steps the master parameters, the moments and the state block equal the restatement BIT FOR BIT, the gradients
   coming from actor_backward / critic_backward: an actor with tanh, an actor with relu and no feature LayerNorm (its ln0 entries are
   left alone), the critic with both; weight decay 0 and 0.01, clipping active, inactive and off; grad_norm = sqrt(sq_norm) to the bit;
2. pack coherence -- what catches a wrong gather-table entry: a twin engine given set_actor(actor_state_dict()) produces bit-equal
   actor_logits (the evaluate pack), actor_backward gradients (the transposed pack) and rollout_actor actions and logits (the
   closed-loop pack); for the critic critic_values, critic_raw_values and critic_backward; after set_critic_value_norm critic_values
   is raw * scale + shift to the bit;
3. a NaN in the gradient: every buffer and what every packed copy computes keep their bits, skipped = 1, step unchanged, and the next
   clean step equals the restatement;
4. stream order: backward, step, evaluate enqueued without a synchronisation equal the same calls with one after each;
5. a deep copy after two steps carries parameters and optimiser state: copy and original take one more step and agree bit for bit;
6. the fixture the reference wrote (tests/golden/optim/optim.npz): three actor_update / critic_update calls within 8 x (the distance
   of the reference's own fp32 results from its fp64 results);
7. the loop closed on collect(20): five critic_update calls and five actor_update calls per agent lower the loss (over the five and at
   the first; Adam's momentum overshoots in between, in torch fp64 as on the device), follow torch fp64's losses to 1e-4 and stay
   within 8 x torch fp32's own distance of a torch fp64 run of the same steps; a HAPPO-style iteration of collect, actor_update,
   critic_update and set_critic_value_norm under torch's synchronisation guard; the vector env's delegates; every refusal a ValueError
   with the network set before still in force.
   Observed ratios: DESIGN.md section 4.31."""
import copy
import math

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import actor_grad_ref as AG
from tests import actor_ref as AR
from tests import critic_grad_ref as GR
from tests import critic_ref as CR
from tests import optim_ref as O
from tests.plan_util import refused

pytestmark = pytest.mark.gpu

N, T_ROWS = 40, 37
MARGIN = 8.0
LR, BETAS, EPS = 5e-4, (0.9, 0.999), 1e-5
CLIPS = {"active": 1e-3, "inactive": 1e6, "off": None}
CHECK_AT = (1, 2, 3, 10)
KINDS = [("actor", "tanh", True), ("actor", "relu", False), ("critic", "tanh", True), ("critic", "relu", False)]
SLOT = 1


@pytest.fixture(scope="module")
def eng():
    e = AR.engine(N, False)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rows(seed, width):
    """37 x 40 stored rows of the fixtures' kind"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T_ROWS, N, width)).astype(np.float32)
    x[1::3, :, 20:] = 0.0
    return x


class Net:
    """one network on an engine behind the same few calls, actor or critic: set, backward over the stored rows with fresh
    coefficients, step, read back"""

    def __init__(self, e, kind, activation, feature_norm, seed=700):
        import torch
        self.e, self.kind, self.activation, self.feature_norm = e, kind, activation, feature_norm
        self.actor = kind == "actor"
        self.n = L.ACTOR_N_PARAMS if self.actor else L.CRITIC_N_PARAMS
        self.first = 0 if feature_norm else 2 * (26 if self.actor else 29)
        self.which = SLOT if self.actor else "critic"
        if self.actor:
            self.sd = {k: v.detach().numpy().copy() for k, v in AR.torch_actor(seed, activation, feature_norm=feature_norm).state_dict().items()}
        else:
            self.sd = {k: v.numpy().copy() for k, v in CR.make_critic(seed, feature_norm).items()}
        self.x = torch.from_numpy(rows(seed + 1, 26 if self.actor else 29)).to(e.device)
        self.actions = torch.from_numpy(np.random.default_rng(seed + 2).integers(0, 3, (T_ROWS, N)).astype(np.int32)).to(e.device)
        self.set()

    def set(self, e=None, sd=None):
        e, sd = e or self.e, sd or self.sd
        if self.actor:
            e.set_actor(SLOT, dict(sd, activation=self.activation))
        else:
            e.set_critic(sd, CR.VALUE_NORM, self.activation)

    def coef(self, i):
        import torch
        c = (np.random.default_rng(5000 + i).standard_normal((T_ROWS, N)) / (T_ROWS * N)).astype(np.float32)
        c[3::7] = 0.0
        return torch.from_numpy(c).to(self.e.device)

    def backward(self, i, e=None):
        e = e or self.e
        if self.actor:
            return e.actor_backward(SLOT, self.x, self.actions, self.coef(i), dent=-0.01 / (T_ROWS * N), per_agent=False)
        return e.critic_backward(self.x, self.coef(i))

    def step(self, grads, e=None, **kw):
        e = e or self.e
        return e.actor_adam_step(SLOT, grads, **kw) if self.actor else e.critic_adam_step(grads, **kw)

    def params(self, e=None):
        """the master copy as sdc_get_* hands it back: fp32 [n]"""
        e = e or self.e
        p = e._host_actors()[SLOT] if self.actor else e._host_critic()
        return np.frombuffer(bytes(p), np.float32, self.n).copy()

    def forward(self, e=None):
        """what the evaluate pack computes over the stored rows"""
        e = e or self.e
        return e.actor_logits(SLOT, self.x, per_agent=False) if self.actor else e.critic_raw_values(self.x)


def state_of(st):
    return {k: st[k] for k in ("step", "beta1_pow", "beta2_pow", "skipped")}


def assert_equals_restatement(net, p, m, v, st, where):
    got = net.e.optim_state(net.which)
    assert np.array_equal(bits(net.params()), bits(p)), where
    assert np.array_equal(bits(got["m"]), bits(m)) and np.array_equal(bits(got["v"]), bits(v)), where
    assert state_of(got) == st, (where, state_of(got), st)


# ---- 1. bit for bit against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", sorted(CLIPS))
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("kind,activation,feature_norm", KINDS)
def test_steps_equal_the_restatement_bit_for_bit(eng, kind, activation, feature_norm, wd, clip):
    net = Net(eng, kind, activation, feature_norm)
    p = net.params()
    m, v, st = np.zeros_like(p), np.zeros_like(p), O.new_state()
    assert_equals_restatement(net, p, m, v, st, "a new network has a new optimiser")
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, max_grad_norm=CLIPS[clip])
    clipped = []
    for i in range(1, max(CHECK_AT) + 1):
        grads = net.backward(i)
        norm = net.step(grads, **kw)
        if i not in CHECK_AT:
            g = grads.flat.cpu().numpy()
            p, m, v, _ = O.step(g, p, m, v, st, first=net.first, **kw)
            continue
        g, sq = grads.flat.cpu().numpy(), float(grads.sq_norm.cpu())
        assert not g[:net.first].any()      # (the backward's contract: exact zeros for a feature LayerNorm that is off)
        p, m, v, want_norm = O.step(g, p, m, v, st, first=net.first, **kw)
        assert float(norm.cpu()) == math.sqrt(sq) == want_norm and sq == O.grad_sq(g), (i, float(norm.cpu()), math.sqrt(sq))
        clipped.append(CLIPS[clip] is not None and CLIPS[clip] / (want_norm + 1e-6) < 1.0)
        assert_equals_restatement(net, p, m, v, st, "after %d steps" % i)
    assert all(clipped) == (clip == "active") and any(clipped) == (clip == "active")
    assert st["step"] == 10 and np.isfinite(p).all()
    if net.first:
        assert np.array_equal(bits(p[:net.first]), bits(np.zeros(net.first)))      # (ln0 as set_* left it: untouched under weight decay)


# ---- 2. pack coherence ------------------------------------------------------------------------------------------------------------------
def twin_engine():
    return AR.engine(N, False)


@pytest.mark.parametrize("activation,feature_norm", [("tanh", True), ("relu", False)])
def test_actor_packs_follow_the_master_copy(activation, feature_norm):
    import torch
    nets = [AR.torch_actor(310 + a, activation, feature_norm=feature_norm) for a in range(3)]
    # (two fresh engines: both samplers stand at their first episode, so the closed loops draw alike)
    mine, twin = twin_engine(), twin_engine()
    try:
        AR.set_actors(mine, nets, activation)
        net = Net(mine, "actor", activation, feature_norm)
        for i in range(1, 4):
            net.step(net.backward(i), lr=1e-2, weight_decay=0.01, max_grad_norm=1e-3)
        AR.set_actors(twin, nets, activation)
        sd = mine.actor_state_dict(SLOT)
        assert set(sd) == set(net.sd) and all(tuple(sd[k].shape) == net.sd[k].shape for k in sd)
        assert max(float(np.abs(sd[k].numpy() - net.sd[k]).max()) for k in sd) > 1e-3      # (the steps moved it)
        twin.set_actor(SLOT, dict(sd, activation=activation))
        assert np.array_equal(bits(net.params(twin)), bits(net.params()))
        assert torch.equal(net.forward(twin).cpu(), net.forward().cpu())                     # SdcActorEvalDev
        g1, g2 = net.backward(7), net.backward(7, twin)
        assert torch.equal(g1.flat.cpu(), g2.flat.cpu()) and torch.equal(g1.sq_norm.cpu(), g2.sq_norm.cpu())      # SdcActorGradDev
        mine.reset()
        twin.reset()
        a, b = mine.rollout_actor(5, sample=True, want_logits=True), twin.rollout_actor(5, sample=True, want_logits=True)      # SdcActorDev
        assert torch.equal(a[5].cpu(), b[5].cpu()) and torch.equal(a[6].cpu(), b[6].cpu()) and torch.equal(a[0].cpu(), b[0].cpu())
        # ... and they differ from what the network set before the steps plays
        twin.set_actor(SLOT, dict(net.sd, activation=activation))
        assert not torch.equal(net.forward(twin).cpu(), net.forward().cpu())
        twin.reset()
        mine.reset()
        a, b = mine.rollout_actor(5, sample=True, want_logits=True), twin.rollout_actor(5, sample=True, want_logits=True)
        assert not torch.equal(a[6][..., SLOT, :].cpu(), b[6][..., SLOT, :].cpu())
    finally:
        mine.close()
        twin.close()


@pytest.mark.parametrize("activation,feature_norm", [("tanh", True), ("relu", False)])
def test_critic_packs_follow_the_master_copy(eng, activation, feature_norm):
    import torch
    from dc_rl_amd.engine import value_norm_scale_shift
    net = Net(eng, "critic", activation, feature_norm)
    for i in range(1, 4):
        net.step(net.backward(i), lr=1e-2, weight_decay=0.01, max_grad_norm=1e-3)
    twin = twin_engine()
    try:
        sd = eng.critic_state_dict()
        assert set(sd) == set(net.sd) and tuple(sd["v_out.weight"].shape) == (1, 64) and tuple(sd["v_out.bias"].shape) == (1,)
        twin.set_critic(sd, CR.VALUE_NORM, activation)
        assert np.array_equal(bits(net.params(twin)), bits(net.params()))
        assert (float(eng._host_critic().scale), float(eng._host_critic().shift)) == (float(twin._critic.scale), float(twin._critic.shift))
        assert torch.equal(eng.critic_values(net.x).cpu(), twin.critic_values(net.x).cpu())              # SdcCriticDev, scale and shift
        assert torch.equal(net.forward(twin).cpu(), net.forward().cpu())
        mine, theirs = net.backward(7), net.backward(7, twin)
        assert torch.equal(mine.flat.cpu(), theirs.flat.cpu()) and torch.equal(mine.sq_norm.cpu(), theirs.sq_norm.cpu())      # SdcCriticGradDev
        twin.set_critic(net.sd, CR.VALUE_NORM, activation)
        assert not torch.equal(net.forward(twin).cpu(), net.forward().cpu())
        # the ValueNorm alone: stream-ordered, the parameters stay
        before = net.params()
        for value_norm in ((0.3, 1e-2), (-3.0, 7.5 ** 2), None):
            eng.set_critic_value_norm(value_norm)
            scale, shift = (np.float32(s) for s in value_norm_scale_shift(value_norm))
            raw = net.forward().cpu().numpy()
            assert np.array_equal(bits(eng.critic_values(net.x).cpu().numpy()), bits(raw * scale + shift)), value_norm
            assert (np.float32(eng._critic.scale), np.float32(eng._critic.shift)) == (scale, shift)
            hc = eng._host_critic()
            assert (np.float32(hc.scale), np.float32(hc.shift)) == (scale, shift)
        assert np.array_equal(bits(net.params()), bits(before))
    finally:
        twin.close()


# ---- 3. a gradient that is not finite ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,activation,feature_norm", [KINDS[0], KINDS[3]])
def test_a_nan_gradient_changes_nothing_but_skipped(eng, kind, activation, feature_norm):
    import torch
    net = Net(eng, kind, activation, feature_norm)
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=0.01, max_grad_norm=1e-3)
    p = net.params()
    m, v, st = np.zeros_like(p), np.zeros_like(p), O.new_state()
    g1 = net.backward(1)
    net.step(g1, **kw)
    p, m, v, _ = O.step(g1.flat.cpu().numpy(), p, m, v, st, first=net.first, **kw)
    fwd, bwd = net.forward().clone(), net.backward(9).flat.clone()
    if net.actor:
        values = None
    else:
        values = eng.critic_values(net.x).clone()
    bad = net.backward(2).flat.clone()
    bad[net.n - 2] = float("nan")      # (a data value)
    norm = net.step(bad, **kw)
    assert math.isnan(float(norm.cpu()))
    st["skipped"] = 1
    assert_equals_restatement(net, p, m, v, st, "after the skipped step")
    assert torch.equal(net.forward(), fwd) and torch.equal(net.backward(9).flat, bwd)
    if values is not None:
        assert torch.equal(eng.critic_values(net.x), values)
    g3 = net.backward(3)
    net.step(g3, **kw)
    p, m, v, _ = O.step(g3.flat.cpu().numpy(), p, m, v, st, first=net.first, **kw)
    assert st == dict(step=2, beta1_pow=0.9 * 0.9, beta2_pow=0.999 * 0.999, skipped=1)
    assert_equals_restatement(net, p, m, v, st, "the next clean step")


# ---- 4. stream order ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,activation,feature_norm", [KINDS[0], KINDS[2]])
def test_backward_step_evaluate_are_stream_ordered(eng, kind, activation, feature_norm):
    import torch
    net = Net(eng, kind, activation, feature_norm)
    kw = dict(lr=1e-2, max_grad_norm=1e-3)
    outs = []
    for i in (1, 2):      # (nothing synchronises between these launches: no .cpu(), no get)
        net.step(net.backward(i), **kw)
        outs.append(net.forward())
    twin = twin_engine()
    try:
        net.set(twin)
        for i in (1, 2):
            g = net.backward(i, twin)
            torch.cuda.synchronize(twin.device)
            net.step(g, twin, **kw)
            torch.cuda.synchronize(twin.device)
            f = net.forward(twin)
            torch.cuda.synchronize(twin.device)
            assert torch.equal(f.cpu(), outs[i - 1].cpu()), i
        assert np.array_equal(bits(net.params(twin)), bits(net.params()))
    finally:
        twin.close()


# ---- 5. a deep copy carries the stepped parameters and the optimiser state ------------------------------------------------------------------
def test_deep_copy_after_two_steps():
    import torch
    from tests.test_gpu_actor_stats import _vec
    v = _vec(N)
    try:
        v.reset()
        nets = [AR.torch_actor(320 + a) for a in range(3)]
        for a in range(3):
            v.set_actor(a, nets[a].state_dict())
        v.set_critic(CR.make_critic(23), CR.VALUE_NORM)
        dev = v.engine.device
        flat = lambda n, seed: torch.from_numpy(np.random.default_rng(seed).standard_normal(n).astype(np.float32) * 1e-2).to(dev)
        kw = dict(lr=1e-3, weight_decay=0.01, max_grad_norm=0.5)
        for i in range(2):
            v.actor_adam_step(SLOT, flat(L.ACTOR_N_PARAMS, 40 + i), **kw)
            v.critic_adam_step(flat(L.CRITIC_N_PARAMS, 50 + i), **kw)
        v.set_critic_value_norm((0.25, 4.0))
        c = copy.deepcopy(v)
        try:
            for w in (v, c):
                d = w.engine.device
                w.actor_adam_step(SLOT, flat(L.ACTOR_N_PARAMS, 60).to(d), **kw)
                w.critic_adam_step(flat(L.CRITIC_N_PARAMS, 61).to(d), **kw)
            for which, sd_of in ((SLOT, lambda w: w.actor_state_dict(SLOT)), ("critic", lambda w: w.critic_state_dict())):
                a, b = sd_of(v), sd_of(c)
                assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a), which
                sa, sb = v.optim_state(which), c.optim_state(which)
                assert np.array_equal(bits(sa["m"]), bits(sb["m"])) and np.array_equal(bits(sa["v"]), bits(sb["v"])), which
                assert state_of(sa) == state_of(sb) and sa["step"] == 3 and sa["m"].any(), which
            assert (c.engine._host_critic().scale, c.engine._host_critic().shift) == (v.engine._host_critic().scale, v.engine._host_critic().shift) == (2.0, 0.25)
            # the untouched actors went along as they were, with a new optimiser
            assert c.optim_state(0)["step"] == 0 and all(torch.equal(c.actor_state_dict(0)[k], v.actor_state_dict(0)[k]) for k in c.actor_state_dict(0))
        finally:
            c.close()
    finally:
        v.close()


# ---- 6. the fixture the reference wrote, on the device ---------------------------------------------------------------------------------------
def _stored_batch(t, dev, **given):
    """an OnPolicyBatch of T = 1 step holding the given fields (the others None); the advantages pass normalized_advantages unchanged"""
    from dc_rl_amd.engine import OnPolicyBatch
    fields = dict.fromkeys(OnPolicyBatch.FIELDS)
    fields.update(given, adv_mean=t.zeros((), dtype=t.float64, device=dev), adv_std=t.ones((), dtype=t.float64, device=dev) - 1e-5)
    return OnPolicyBatch(**fields)


def test_three_updates_on_the_fixtures_inputs():
    import torch as t
    fx, hyper = O.fixture(), O.fixture_hyper()
    R = AG.R
    e = AR.engine(R, False)      # (one step of 67 envs: the fixtures' 67 rows)
    try:
        dev = e.device
        kw = dict(lr=hyper["lr"], betas=hyper["betas"], eps=hyper["eps"], weight_decay=hyper["weight_decay"], max_grad_norm=hyper["max_grad_norm"])
        # the actor
        act, fn, c = O.actor_case()
        a = 1
        e.set_actor(a, dict(c["sd"], activation=act))
        col = lambda x, dt: t.zeros((1, R, 3), dtype=dt, device=dev).index_copy_(2, t.tensor([a], device=dev), t.from_numpy(x).to(dev).view(1, R, 1))
        obs = t.zeros((2, R, 3, 26), device=dev)
        obs[0, :, a] = t.from_numpy(c["obs"]).to(dev)
        adv = t.from_numpy(c["advantages"]).to(dev).view(1, R)
        b = _stored_batch(t, dev, obs=obs, actions=col(c["actions"].astype(np.int32), t.int32), action_log_probs=col(c["old_log_probs"], t.float32),
                          advantages=adv)
        assert t.equal(b.normalized_advantages(), adv)
        factor = t.from_numpy(c["factor"]).to(dev).view(1, R).contiguous()
        results = []
        for u in range(O.UPDATES):
            _, norm = e.actor_update(b, a, float(fx["clip_param"]), float(fx["entropy_coef"]), factor=factor, **kw)
            assert abs(float(norm.cpu()) - float(fx["actor_grad_norm32"][u])) <= 1e-4 * float(norm.cpu())
            results.append(O.sd_flat({k: v.numpy() for k, v in e.actor_state_dict(a).items()}, AG.FIELDS, AG.KEYS, AG.SHAPES))
        d, d32 = O.fixture_distance(results, "actor")
        print("actor_update x 3: %.3e from the reference's fp64 results, the reference's fp32 results %.3e: ratio %.2f" % (d, d32, d / d32))
        assert d <= MARGIN * d32
        # the critic, its ValueNorm the one the reference's update u normalised the returns with
        act, fn, c = O.critic_case()
        e.set_critic(c["sd"], None, act)
        share = t.zeros((2, R, 29), device=dev)
        share[0] = t.from_numpy(c["share_obs"]).to(dev)
        vp = t.zeros((2, R), device=dev)
        vp[0] = t.from_numpy(c["value_preds"][:, 0]).to(dev)
        b = _stored_batch(t, dev, share_obs=share, value_preds=vp, returns=t.from_numpy(c["returns"][:, 0].copy()).to(dev).view(1, R),
                          actions=t.zeros((1, R, 3), dtype=t.int32, device=dev))
        results = []
        for u in range(O.UPDATES):
            _, norm = e.critic_update(b, float(fx["clip_param"]), float(fx["huber_delta"]), True, True, float(fx["value_loss_coef"]),
                                      value_norm=(fx["critic_norm_mean"][u], fx["critic_norm_var"][u]), **kw)
            assert abs(float(norm.cpu()) - float(fx["critic_grad_norm32"][u])) <= 1e-4 * float(norm.cpu())
            results.append(O.sd_flat({k: v.numpy() for k, v in e.critic_state_dict().items()}, GR.FIELDS, GR.KEYS, GR.SHAPES))
        d, d32 = O.fixture_distance(results, "critic")
        print("critic_update x 3: %.3e from the reference's fp64 results, the reference's fp32 results %.3e: ratio %.2f" % (d, d32, d / d32))
        assert d <= MARGIN * d32 and not fn and not results[-1][:58].any()
    finally:
        e.close()


# ---- 7. the loop closed on collect(20) ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def looped():
    """an engine with three tanh actors and a critic under a ValueNorm, and a batch of 20 steps collected with them"""
    e = AR.engine(N, False)
    nets = [AR.torch_actor(300 + a) for a in range(3)]
    AR.set_actors(e, nets)
    sd = CR.make_critic(21)
    e.set_critic(sd, CR.VALUE_NORM)
    e.reset()
    batch = e.collect(20)
    yield e, nets, sd, batch
    e.close()


def torch_adam_run(net, loss_of, steps, lr, max_norm):
    """`steps` Adam steps behind clip_grad_norm_ on the module -> (the losses before each step and after the last, the module)"""
    import torch
    opt = torch.optim.Adam(net.parameters(), lr=lr, betas=BETAS, eps=EPS, foreach=False, fused=False)
    losses = []
    for s in range(steps + 1):
        opt.zero_grad()
        loss = loss_of(net)
        losses.append(float(loss.detach()))
        if s == steps:
            break
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm, foreach=False)
        opt.step()
    return losses, net


def param_distance(sd_a, sd_b):
    return max(float((sd_a[k].double() - sd_b[k].double()).abs().max()) for k in sd_a)


LOSS_BAR = 1e-4      # (the networks' outputs agree with fp64 to 2e-4, the project's bar for them; a loss averages 800 rows of them)


def loss_falls(losses, losses64, who):
    """The loss falls over the five steps and at the first of them, and follows a torch fp64 run of the same steps.  Adam is no descent
    method step by step -- its momentum overshoots, in torch fp64 at the same steps as on the device -- so
    unlike the SGD steps of sections 4.28 and 4.30 a rise in between is not held against it; the first step (m = g, v = g^2: a
    sign-descent step of size lr) must descend."""
    assert losses[-1] < losses[0] and losses[1] < losses[0], (who, losses)
    assert losses64[-1] < losses64[0]
    gap = max(abs(a - b) for a, b in zip(losses, losses64))
    assert gap <= LOSS_BAR, (who, gap)


def test_updates_close_the_loop(looped):
    import torch
    from dc_rl_amd.engine import value_norm_scale_shift
    from tests.test_gpu_actor_grad import _torch_loss
    e, nets, csd, b = looped
    T, clip, coef_ent, delta, steps, max_norm = b.n_steps, 0.2, 0.01, 10.0, 5, 10.0
    scale, shift = value_norm_scale_shift(CR.VALUE_NORM)
    adv = b.normalized_advantages().reshape(-1).cpu()
    try:
        # the critic
        x = b.share_obs[:T].reshape(T * N, 29).cpu()
        vp, ret = b.value_preds[:T].reshape(-1).cpu(), b.returns.reshape(-1).cpu()
        losses = []
        for s in range(steps):
            terms, norm = e.critic_update(b, clip, delta, lr=LR, eps=EPS, max_grad_norm=max_norm)
            losses.append(terms.summary()["value_loss"])
            assert norm.dim() == 0 and norm.dtype == torch.float64 and float(norm.cpu()) > 0.0
        losses.append(e.critic_grads(b, clip, delta)[1].summary()["value_loss"])
        vloss = lambda net: GR.torch_value_loss(net(x.to(next(net.parameters()).dtype)), vp.to(next(net.parameters()).dtype),
                                                ret.to(next(net.parameters()).dtype), scale, shift, clip, delta, 3).mean()
        sd0 = {k: np.asarray(v) for k, v in csd.items()}
        l64, n64 = torch_adam_run(GR.torch_net(sd0, "tanh", torch.float64), vloss, steps, LR, max_norm)
        l32, n32 = torch_adam_run(GR.torch_net(sd0, "tanh", torch.float32), vloss, steps, LR, max_norm)
        d_dev, d_32 = param_distance(e.critic_state_dict(), n64.state_dict()), param_distance(n32.state_dict(), n64.state_dict())
        print("critic: value loss %s (torch fp64 %s); parameters %.3e from torch fp64, torch fp32 %.3e: ratio %.2f" %
              (losses, l64, d_dev, d_32, d_dev / d_32))
        loss_falls(losses, l64, "critic")
        assert d_dev <= MARGIN * d_32
        assert state_of(e.optim_state("critic")) == dict(step=steps, beta1_pow=pytest.approx(0.9 ** steps), beta2_pow=pytest.approx(0.999 ** steps),
                                                         skipped=0)
        # the three actors, each against the batch's stored log-probabilities (factor None: ones)
        for a in range(3):
            xa = b.obs[:T, :, a].reshape(T * N, 26).cpu()
            acts = b.actions[..., a].reshape(-1).cpu()
            old = b.action_log_probs[..., a].reshape(-1).cpu()
            losses = []
            for s in range(steps):
                terms, norm = e.actor_update(b, a, clip, coef_ent, lr=LR, eps=EPS, max_grad_norm=max_norm)
                sm = terms.summary()
                losses.append(sm["policy_loss"] - coef_ent * sm["entropy"])
            sm = e.actor_update_terms(b, a, clip).summary()
            losses.append(sm["policy_loss"] - coef_ent * sm["entropy"])
            aloss = lambda net: _torch_loss(net, xa, acts, old, adv, clip, coef_ent)
            l64, n64 = torch_adam_run(copy.deepcopy(nets[a]).double(), aloss, steps, LR, max_norm)
            l32, n32 = torch_adam_run(copy.deepcopy(nets[a]), aloss, steps, LR, max_norm)
            d_dev, d_32 = param_distance(e.actor_state_dict(a), n64.state_dict()), param_distance(n32.state_dict(), n64.state_dict())
            print("actor %d: loss %s (torch fp64 %s); parameters %.3e from torch fp64, torch fp32 %.3e: ratio %.2f" %
                  (a, losses, l64, d_dev, d_32, d_dev / d_32))
            loss_falls(losses, l64, "actor %d" % a)
            assert d_dev <= MARGIN * d_32, a
    finally:
        AR.set_actors(e, nets)
        e.set_critic(csd, CR.VALUE_NORM)


def test_a_happo_iteration_never_waits_for_the_host(looped):
    """collect -> actor_update per agent with the HAPPO factor -> critic_update -> set_critic_value_norm -> collect: torch's
    synchronisation guard stands over everything between the first and the last launch; the logged scalars are read afterwards"""
    import torch
    e, nets, csd, _ = looped
    try:
        e.reset()
        torch.cuda.synchronize(e.device)
        torch.cuda.set_sync_debug_mode("error")
        try:
            b = e.collect(20)
            logged, factor = [], None
            for a in (2, 0, 1):
                terms, norm = e.actor_update(b, a, 0.2, 0.01, factor=factor, lr=LR, max_grad_norm=10.0)
                after = e.actor_update_terms(b, a, 0.2, factor=factor)      # (the runner's second evaluation: the next agent's factor)
                factor = after.factor
                logged += [terms.stats, norm]
            terms, norm = e.critic_update(b, lr=LR, max_grad_norm=10.0)
            logged += [terms.stats, norm]
            e.set_critic_value_norm((0.1, 2.0))
            b2 = e.collect(20)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize(e.device)
        assert all(bool(torch.isfinite(x).all()) for x in logged) and bool(torch.isfinite(b2.returns).all())
        assert [e.optim_state(a)["step"] for a in range(3)] == [1, 1, 1] and e.optim_state("critic")["step"] == 1
        assert not torch.equal(b.logits, b2.logits)
    finally:
        AR.set_actors(e, nets)
        e.set_critic(csd, CR.VALUE_NORM)


def test_vec_env_delegates_return_the_same_tensors(looped):
    import torch
    from tests.test_gpu_actor_stats import _vec
    e, nets, csd, b = looped
    v = _vec(N)
    try:
        v.reset()
        for a in range(3):
            v.set_actor(a, nets[a].state_dict())
        v.set_critic(csd, CR.VALUE_NORM)
        assert v.engine.device == e.device
        kw = dict(lr=LR, max_grad_norm=10.0)
        ta, na = e.actor_update(b, SLOT, 0.2, 0.01, **kw)
        tv, nv = v.actor_update(b, SLOT, 0.2, 0.01, **kw)
        assert torch.equal(ta.stats, tv.stats) and torch.equal(na, nv)
        tc, nc = e.critic_update(b, **kw)
        tw, nw = v.critic_update(b, **kw)
        assert torch.equal(tc.stats, tw.stats) and torch.equal(tc.dvalue, tw.dvalue) and torch.equal(nc, nw)
        ga, gc = e.actor_grads(b, SLOT)[0], e.critic_grads(b)[0]
        assert torch.equal(e.actor_adam_step(SLOT, ga, **kw), v.actor_adam_step(SLOT, v.actor_grads(b, SLOT)[0], **kw))
        assert torch.equal(e.critic_adam_step(gc.flat, **kw), v.critic_adam_step(v.critic_grads(b)[0].flat, **kw))
        for mine, theirs in ((e.actor_state_dict(SLOT), v.actor_state_dict(SLOT)), (e.critic_state_dict(), v.critic_state_dict())):
            assert set(mine) == set(theirs) and all(torch.equal(mine[k], theirs[k]) for k in mine)
        for which in (SLOT, "critic"):
            sa, sb = e.optim_state(which), v.optim_state(which)
            assert np.array_equal(bits(sa["m"]), bits(sb["m"])) and state_of(sa) == state_of(sb) and sa["step"] == 2
        v.load_optim_state(SLOT, e.optim_state(SLOT))
        v.set_critic_value_norm((0.5, 9.0))
        assert (v.engine._host_critic().scale, v.engine._host_critic().shift) == (3.0, 0.5)
    finally:
        v.close()
        AR.set_actors(e, nets)
        e.set_critic(csd, CR.VALUE_NORM)


def test_every_refusal_reaches_python_and_the_network_stays(looped):
    import torch
    e, nets, csd, b = looped
    dev = e.device
    ga, gc = torch.zeros(L.ACTOR_N_PARAMS, device=dev), torch.zeros(L.CRITIC_N_PARAMS, device=dev)
    before = (e.actor_state_dict(0), e.critic_state_dict(), e.optim_state(0), e.optim_state("critic"))
    logits = e.actor_logits(0, b.obs[:3], per_agent=True).clone()
    for who, step in (("sdc_actor_adam_step", lambda **kw: e.actor_adam_step(0, ga, **kw)), ("sdc_critic_adam_step", lambda **kw: e.critic_adam_step(gc, **kw))):
        refused(e, who + ": lr must be finite and not negative", lambda: step(lr=-1.0))
        refused(e, who + ": lr must be finite and not negative", lambda: step(lr=float("inf")))
        refused(e, who + r": beta1 and beta2 must lie in \[0, 1\)", lambda: step(lr=LR, betas=(1.0, 0.999)))
        refused(e, who + r": beta1 and beta2 must lie in \[0, 1\)", lambda: step(lr=LR, betas=(0.9, -0.1)))
        refused(e, who + ": eps must be finite and not negative", lambda: step(lr=LR, eps=-1e-8))
        refused(e, who + ": weight_decay must be finite and not negative", lambda: step(lr=LR, weight_decay=float("nan")))
        refused(e, who + ": max_grad_norm must be above 0", lambda: step(lr=LR, max_grad_norm=0.0))
        refused(e, who + ": max_grad_norm must be above 0", lambda: step(lr=LR, max_grad_norm=float("nan")))
    p = lambda x: x.data_ptr()
    import ctypes as C
    adam = L.SdcAdam(lr=LR, beta1=0.9, beta2=0.999, eps=EPS, weight_decay=0.0, max_grad_norm=10.0)
    norm = torch.zeros(2, dtype=torch.float64, device=dev)
    raw = lambda **kw: e._call(e.lib.sdc_actor_adam_step, kw.get("slot", 0), kw.get("g", p(ga)), kw.get("adam", C.byref(adam)), kw.get("norm", p(norm)),
                               e._stream(), refuses=True)
    refused(e, r"sdc_actor_adam_step: agent_slot = 3 outside \[0, 2\]", lambda: raw(slot=3))
    refused(e, "sdc_actor_adam_step: null grads", lambda: raw(g=None))
    refused(e, "sdc_actor_adam_step: grads not dword-aligned", lambda: raw(g=p(ga) + 2))
    refused(e, "sdc_actor_adam_step: grad_norm not 8-byte aligned", lambda: raw(norm=p(norm) + 4))
    refused(e, "sdc_actor_adam_step: null sdc_adam", lambda: raw(adam=None))
    refused(e, "sdc_set_critic_norm: scale must be positive", lambda: e.set_critic_value_norm((0.0, 0.0)))
    refused(e, "sdc_set_critic_norm: an entry that is not finite", lambda: e.set_critic_value_norm((float("inf"), 1.0)))
    st = e.optim_state(0)
    refused(e, "sdc_set_actor_optim: step must not be negative", lambda: e.load_optim_state(0, dict(st, step=-1)))
    refused(e, r"sdc_set_actor_optim: beta1_pow and beta2_pow must lie in \(0, 1\]", lambda: e.load_optim_state(0, dict(st, beta1_pow=0.0)))
    refused(e, r"sdc_set_critic_optim: beta1_pow and beta2_pow must lie in \(0, 1\]",
            lambda: e.load_optim_state("critic", dict(e.optim_state("critic"), beta2_pow=1.5)))
    bad_v = st["v"].copy()
    bad_v[5] = -1.0
    refused(e, "sdc_set_actor_optim: a moment that is not finite, or a negative v", lambda: e.load_optim_state(0, dict(st, v=bad_v)))
    # the Python side's own checks, in its words
    refused(e, r"actor_adam_step: grads must be", lambda: e.actor_adam_step(0, gc, lr=LR))
    refused(e, r"critic_adam_step: grads must be", lambda: e.critic_adam_step(gc.double(), lr=LR))
    refused(e, "actor_adam_step: agent = 3 must be 0", lambda: e.actor_adam_step(3, ga, lr=LR))
    refused(e, "actor_adam_step: lr = 'x' must be a number", lambda: e.actor_adam_step(0, ga, lr="x"))
    refused(e, "critic_adam_step: betas = 0.9 must be a pair", lambda: e.critic_adam_step(gc, lr=LR, betas=0.9))
    refused(e, "optim_state: which = 'actor' must be", lambda: e.optim_state("actor"))
    refused(e, r"load_optim_state: m has shape \(3,\)", lambda: e.load_optim_state(0, dict(st, m=np.zeros(3, np.float32))))
    with pytest.raises(TypeError):
        e.actor_update(b, 0)      # (lr has no default)
    # before the network is set: the library's text
    fresh = AR.engine(N, False)
    try:
        fa, fc = ga.to(fresh.device), gc.to(fresh.device)
        for match, call in (("sdc_actor_adam_step: no actor is set for agent_slot 0", lambda: fresh.actor_adam_step(0, fa, lr=LR)),
                            ("sdc_critic_adam_step: sdc_set_critic first", lambda: fresh.critic_adam_step(fc, lr=LR)),
                            ("sdc_get_actor_optim: no actor is set for agent_slot 2", lambda: fresh.optim_state(2)),
                            ("sdc_get_critic_optim: sdc_set_critic first", lambda: fresh.optim_state("critic")),
                            ("sdc_set_critic_norm: sdc_set_critic first", lambda: fresh.set_critic_value_norm(None)),
                            ("actor_state_dict: no actor is set", lambda: fresh.actor_state_dict(1)),
                            ("critic_state_dict: set_critic first", lambda: fresh.critic_state_dict())):
            with pytest.raises(ValueError, match=match):
                call()
    finally:
        fresh.close()
    # the networks and optimisers set before are still in force, to the bit
    after = (e.actor_state_dict(0), e.critic_state_dict(), e.optim_state(0), e.optim_state("critic"))
    for x, y in zip(before[:2], after[:2]):
        assert all(torch.equal(x[k], y[k]) for k in x)
    for x, y in zip(before[2:], after[2:]):
        assert np.array_equal(bits(x["m"]), bits(y["m"])) and np.array_equal(bits(x["v"]), bits(y["v"])) and state_of(x) == state_of(y)
    assert torch.equal(e.actor_logits(0, b.obs[:3], per_agent=True), logits)
    assert float(e._host_critic().scale) == float(np.float32(value_norm_of(CR.VALUE_NORM)[0]))


def value_norm_of(value_norm):
    from dc_rl_amd.engine import value_norm_scale_shift
    return value_norm_scale_shift(value_norm)
