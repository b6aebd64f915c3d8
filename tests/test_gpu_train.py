"""TRAIN ON THE DEVICE on the MI355X (include/sustaindc_hip.h; dc_rl_amd.SdcEngine.permutation / minibatch / value_norm_update /
happo_train), 40 envs and collect(20) = 800 rows; mini-batches of 400, 200 and 160 rows are no multiples of the 64 rows a workgroup of
the gradient kernels takes:
  1. sdc_permutation equals the NumPy restatement (tests/train_ref.py) bit for bit at every size the code takes another path at;
  2. minibatch equals index_select on every field bit for bit; with agent=1 sentinel values in columns 0 and 2 survive; an index of -1
     and one of T N give zero rows and bad == 1 with the neighbours intact; into= gives the same bits;
  3. value_norm_update equals the restatement bit for bit over 5 updates at n = 1, 63, 800 and 262 144 + 77 (stage 1 wraps); behind it
     critic_values == raw * scale + shift to the bit and a fresh collect's value_preds follow; value_loss through
     sdc_value_loss_normed equals sdc_value_loss given the read-back scale and shift;
  4. happo_train(indices=) equals the same schedule written out with minibatch, actor_update, actor_update_terms, value_norm_update
     and critic_update -- parameters, moments, state blocks and the ValueNorm bit for bit -- and happo_train(seed=) equals
     happo_train(indices= the restatement's permutations);
  5. the fixture the reference's own HAPPO.train and VCritic.train wrote (tests/golden/train/train.npz), replayed with its permutations:
     parameters and (scale, shift) within 8 x the reference's own fp32 distance from its fp64 run;
  6. collect -> happo_train -> collect under torch's synchronisation guard; a deep copy trains on and agrees; every refusal is a
     ValueError that leaves the networks and the ValueNorm as they were."""
import copy
import ctypes as C

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import actor_ref as AR
from tests import critic_ref as CR
from tests import train_ref as TR

pytestmark = pytest.mark.gpu

N, T = 40, 20
LR = 5e-4
VN0 = dict(running_mean=-0.75, running_mean_sq=16.0, debiasing_term=0.25)      # (mean -3, mean_sq 64: var 55)
SCHEDULE = dict(ppo_epoch=2, critic_epoch=2, actor_num_mini_batch=2, critic_num_mini_batch=4, lr=LR, critic_lr=7e-4, max_grad_norm=10.0,
                beta=0.999)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def start(e, nets, csd, vn=VN0):
    AR.set_actors(e, nets)
    e.set_critic(csd, CR.VALUE_NORM)
    e.set_value_norm(vn)


@pytest.fixture(scope="module")
def rig():
    """an engine with three tanh actors, a critic and an installed ValueNorm, and a batch of 20 steps collected with them"""
    e = AR.engine(N, False)
    nets = [AR.torch_actor(400 + a) for a in range(3)]
    csd = CR.make_critic(31)
    start(e, nets, csd)
    e.reset()
    batch = e.collect(T)
    yield e, nets, csd, batch
    e.close()


def training_state(e):
    """everything an update moves, as host arrays: the actors, the critic, every optimiser's state, the ValueNorm"""
    out = {}
    for a in range(3):
        out.update({"actor%d/%s" % (a, k): v.numpy().copy() for k, v in e.actor_state_dict(a).items()})
    out.update({"critic/" + k: v.numpy().copy() for k, v in e.critic_state_dict().items()})
    for which in (0, 1, 2, "critic"):
        st = e.optim_state(which)
        out.update({"optim%s/%s" % (which, k): np.asarray(st[k]) for k in ("m", "v", "step", "beta1_pow", "beta2_pow", "skipped")})
    out.update({"value_norm/" + k: np.float32(v) for k, v in e.value_norm_state().items()})
    return out


def assert_same_state(a, b, where):
    assert set(a) == set(b)
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (where, k)


# ---- 1. the permutation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 800, 1025, 4097, 672 * 4096])
def test_permutation_equals_the_restatement_bit_for_bit(rig, n):
    e = rig[0]
    for seed, stream in ((20260101, (2 << 32) | 3), ((0xDEADBEEF << 32) | 5, 0)):
        got = e.permutation(n, seed, stream)
        assert got.dtype == e.torch.int32 and tuple(got.shape) == (n,)
        assert np.array_equal(got.cpu().numpy(), TR.permutation(n, seed, stream)[0]), (n, seed, stream)
        if n > 1025:
            break      # (one key at the large sizes: the restatement takes seconds there)


# ---- 2. the gather ------------------------------------------------------------------------------------------------------------------------
PER_STEP = ("obs", "share_obs", "actions", "logits", "action_log_probs", "entropy", "rewards", "dones", "masks", "values", "value_preds",
            "returns", "advantages")


def test_minibatch_equals_index_select_on_every_field(rig):
    import torch
    e, _, _, b = rig
    flat = b.flat()
    for rows, stream in ((800, 0), (400, 1), (200, 2), (160, 3), (40, 4)):
        idx = e.permutation(T * N, 5, stream)[:rows]
        factor = torch.rand((T, N), device=e.device)
        mb = e.minibatch(b, idx, factor=factor)
        assert mb.n_steps == rows // N and int(mb.bad.cpu()) == 0
        for name in PER_STEP:
            want = flat[name].index_select(0, idx.long())
            got = getattr(mb, name)
            assert tuple(got.shape) == (rows // N, N) + tuple(want.shape[1:]) and got.dtype == want.dtype, name
            assert torch.equal(got.reshape(want.shape).view(torch.uint8), want.contiguous().view(torch.uint8)), (rows, name)
        assert torch.equal(mb.factor.view(-1), factor.view(-1).index_select(0, idx.long()))
        assert mb.adv_mean is b.adv_mean and mb.adv_std is b.adv_std
        assert torch.equal(mb.normalized_advantages().view(-1), b.normalized_advantages().view(-1).index_select(0, idx.long()))
    # a caller's own index array, with repeats
    idx = torch.randint(0, T * N, (3 * N,), device=e.device, dtype=torch.int32)
    mb = e.minibatch(b, idx)
    assert torch.equal(mb.share_obs.view(-1, 29), flat["share_obs"].index_select(0, idx.long()))


def test_minibatch_of_one_agent_leaves_the_other_columns(rig):
    import torch
    e, _, _, b = rig
    flat = b.flat()
    idx = e.permutation(T * N, 6, 0)[:400]
    mb = e.minibatch(b, idx, agent=1, critic=False)
    assert mb.share_obs is None and mb.returns is None and mb.dones is None and mb.rewards is None
    sentinel = {}
    for name in ("obs", "actions", "logits", "action_log_probs", "entropy"):
        x = getattr(mb, name)
        x.copy_((torch.full_like(x, 7) if x.dtype == torch.int32 else torch.full_like(x, -123.25)))
        sentinel[name] = x.clone()
    again = e.minibatch(b, idx, agent=1, critic=False, into=mb)
    assert again is mb
    for name, s in sentinel.items():
        got, want = getattr(mb, name), flat[name].index_select(0, idx.long()).view(getattr(mb, name).shape)
        assert torch.equal(got[:, :, 1], want[:, :, 1]), name
        for col in (0, 2):
            assert torch.equal(got[:, :, col], s[:, :, col]), (name, col)
    assert torch.equal(mb.advantages.view(-1), flat["advantages"].index_select(0, idx.long()))
    # the critic's fields alone
    mc = e.minibatch(b, idx, actors=False)
    assert mc.obs is None and mc.advantages is None and mc.n_steps == 10
    for name in ("share_obs", "values", "value_preds", "returns"):
        assert torch.equal(getattr(mc, name).view(400, -1), flat[name].index_select(0, idx.long()).view(400, -1)), name


def test_an_index_outside_the_rows_is_never_an_address(rig):
    import torch
    e, _, _, b = rig
    flat = b.flat()
    idx = e.permutation(T * N, 7, 0)[:200].clone()
    idx[17], idx[130] = -1, T * N
    good = torch.ones(200, dtype=torch.bool, device=e.device)
    good[17] = good[130] = False
    mb = e.minibatch(b, idx)
    assert int(mb.bad.cpu()) == 1
    safe = idx.clamp(0, T * N - 1).long()
    for name in PER_STEP:
        got = getattr(mb, name).view(200, -1)
        want = flat[name].index_select(0, safe).view(200, -1)
        assert torch.equal(got[good], want[good]), name
        assert not bool(got[~good].view(torch.uint8).any()), name
    # the flag is cleared by the next call on the same tensors
    idx2 = e.permutation(T * N, 7, 1)[:200]
    assert int(e.minibatch(b, idx2, into=mb).bad.cpu()) == 0
    same = e.minibatch(b, idx2)
    for name in PER_STEP:
        assert torch.equal(getattr(mb, name).view(torch.uint8), getattr(same, name).view(torch.uint8)), name


# ---- 3. ValueNorm -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 800, 262144 + 77])
def test_value_norm_update_equals_the_restatement_bit_for_bit(rig, n):
    import torch
    e, nets, csd, b = rig
    try:
        rng = np.random.default_rng(n)
        st = tuple(np.float32(VN0[k]) for k in ("running_mean", "running_mean_sq", "debiasing_term"))
        share = b.share_obs[:3].contiguous()
        for u in range(5):
            x = (rng.normal(-3.0, 2.0, n) * (1 + 0.3 * u)).astype(np.float32)
            e.value_norm_update(torch.from_numpy(x).to(e.device), 0.999)
            st, (scale, shift) = TR.value_norm_update(st, x, 0.999)
            got = e.value_norm_state()
            want = dict(zip(("running_mean", "running_mean_sq", "debiasing_term", "scale", "shift"), (*st, scale, shift)))
            assert all(bits(got[k]) == bits(want[k]) for k in want), (n, u, got, want)
        # the critic follows: values are raw * scale + shift in fp32, to the bit
        raw = e.critic_raw_values(share)
        assert torch.equal(e.critic_values(share), raw * float(scale) + float(shift))
        p = e._host_critic()
        assert (bits(p.scale), bits(p.shift)) == (bits(scale), bits(shift))
    finally:
        start(e, nets, csd)


def test_collect_and_value_loss_follow_the_device_value_norm(rig):
    import torch
    e, nets, csd, b = rig
    try:
        e.value_norm_update(b.returns, 0.9)
        vn = e.value_norm_state()
        assert e._value_norm_installed and bits(vn["scale"]) != bits(np.sqrt(np.float32(55.0)))
        raw = e.critic_raw_values(b.share_obs[:T])
        normed = e.value_loss(raw, b.value_preds[:T], b.returns)
        # sdc_value_loss given the very scale and shift that were read back
        loss, dvalue, stats = torch.empty_like(raw), torch.empty_like(raw), torch.empty(8, dtype=torch.float64, device=e.device)
        p = lambda x: C.c_void_p(x.data_ptr())
        e._call(e.lib.sdc_value_loss, raw.numel(), p(raw), p(b.value_preds), p(b.returns), vn["scale"], vn["shift"], 0.2, 10.0, 3,
                1.0 / raw.numel(), p(loss), p(dvalue), p(stats), e._stream(), refuses=True)
        assert torch.equal(normed.loss, loss) and torch.equal(normed.dvalue, dvalue) and torch.equal(normed.stats, stats)
        assert bool(loss.any()) and bool(dvalue.any())
        # a fresh collect's value predictions are normalised with the device's statistics
        e.reset()
        b2 = e.collect(T)
        want = (b2.values - np.float32(vn["shift"])) / np.float32(vn["scale"])
        assert torch.allclose(b2.value_preds, want, rtol=1e-6, atol=1e-6)
        assert torch.equal(b2.values, e.critic_raw_values(b2.share_obs) * vn["scale"] + vn["shift"])
        # uninstalled, the critic keeps what it has and the host path is back
        e.set_value_norm(None)
        assert not e._value_norm_installed and (float(e._critic.scale), float(e._critic.shift)) == (vn["scale"], vn["shift"])
        plain = e.value_loss(raw, b.value_preds[:T], b.returns)
        assert torch.equal(plain.loss, loss) and torch.equal(plain.stats, stats)
        with pytest.raises(ValueError, match="no ValueNorm is installed"):
            e.value_norm_update(b.returns)
    finally:
        start(e, nets, csd)
        e.reset()


# ---- 4. happo_train --------------------------------------------------------------------------------------------------------------------------
def written_out(e, b, indices, order=(0, 1, 2), use_factor=True, **s):
    """happo_train's schedule in the calls it is made of"""
    adam = dict(max_grad_norm=s["max_grad_norm"])
    factor, logged = None, []
    for a in order:
        _, old_lp, _ = e.evaluate_actions(b.obs[:T], b.actions, agents=(a,))
        rows = T // s["actor_num_mini_batch"] * N
        for ep in range(s["ppo_epoch"]):
            perm = indices[(a, ep)]
            for k in range(0, T * N, rows):
                mb = e.minibatch(b, perm[k:k + rows], agent=a, critic=False, factor=factor)
                terms, norm = e.actor_update(mb, a, 0.2, 0.01, factor=mb.factor, lr=s["lr"], **adam)
                logged.append((a, terms.stats, norm))
        if use_factor:
            factor = e.actor_update_terms(b, a, 0.2, factor=factor, old_log_probs=old_lp).factor
    rows = T // s["critic_num_mini_batch"] * N
    for ep in range(s["critic_epoch"]):
        perm = indices[("critic", ep)]
        for k in range(0, T * N, rows):
            mb = e.minibatch(b, perm[k:k + rows], actors=False)
            e.value_norm_update(mb.returns, s["beta"])
            terms, norm = e.critic_update(mb, lr=s["critic_lr"], **adam)
            logged.append(("critic", terms.stats, norm))
    return factor, logged


def restated_indices(e, seed, s):
    import torch
    out = {}
    for who, stream_who, epochs in [(a, a, s["ppo_epoch"]) for a in range(3)] + [("critic", 3, s["critic_epoch"])]:
        for ep in range(epochs):
            out[(who, ep)] = torch.from_numpy(TR.permutation(T * N, seed, (stream_who << 32) | ep)[0]).to(e.device)
    return out


def test_happo_train_equals_its_schedule_written_out(rig):
    import torch
    e, nets, csd, b = rig
    try:
        idx = restated_indices(e, 77, SCHEDULE)
        factor, logged = written_out(e, b, idx, order=(2, 0, 1), **SCHEDULE)
        want = training_state(e)
        start(e, nets, csd)
        info = e.happo_train(b, indices=idx, agent_order=(2, 0, 1), **SCHEDULE)
        assert_same_state(training_state(e), want, "indices=")
        assert torch.equal(info.factor, factor)
        mine = [(a, s, n) for a in (2, 0, 1) for s, n in info.actor[a]] + [("critic", s, n) for s, n in info.critic]
        assert len(mine) == len(logged) == 3 * 2 * 2 + 2 * 4
        for (wa, ws, wn), (ga, gs, gn) in zip(logged, mine):
            assert wa == ga and torch.equal(ws, gs) and torch.equal(wn, gn)
        # the seed draws the restatement's permutations
        start(e, nets, csd)
        e.happo_train(b, seed=77, agent_order=(2, 0, 1), **SCHEDULE)
        assert_same_state(training_state(e), want, "seed=")
        # another seed trains on other mini-batches
        start(e, nets, csd)
        e.happo_train(b, seed=78, agent_order=(2, 0, 1), **SCHEDULE)
        assert not np.array_equal(training_state(e)["optimcritic/m"], want["optimcritic/m"])
        # the summary: the reference's train_info means, from the logged statistics
        summ = info.summary()
        ups = [(s.cpu().numpy(), float(n.cpu())) for a, s, n in logged if a == 0]
        assert summ["actor"][0]["policy_loss"] == pytest.approx(np.mean([-s[0] / s[7] for s, _ in ups]), rel=1e-12)
        assert summ["actor"][0]["ratio"] == pytest.approx(np.mean([s[1] / s[7] for s, _ in ups]), rel=1e-12)
        assert summ["actor"][0]["dist_entropy"] == pytest.approx(np.mean([s[3] / s[7] for s, _ in ups]), rel=1e-12)
        assert summ["actor"][0]["actor_grad_norm"] == pytest.approx(np.mean([n for _, n in ups]), rel=1e-12)
        ups = [(s.cpu().numpy(), float(n.cpu())) for a, s, n in logged if a == "critic"]
        assert summ["critic"]["value_loss"] == pytest.approx(np.mean([s[0] / s[7] for s, _ in ups]), rel=1e-12)
        assert summ["critic"]["critic_grad_norm"] == pytest.approx(np.mean([n for _, n in ups]), rel=1e-12)
        assert set(summ["actor"]) == {0, 1, 2} and all(np.isfinite(list(v.values())).all() for v in summ["actor"].values())
    finally:
        start(e, nets, csd)


def test_happo_train_without_factor_or_value_norm_updates(rig):
    e, nets, csd, b = rig
    try:
        s = dict(SCHEDULE, ppo_epoch=1, critic_epoch=1, actor_num_mini_batch=5, critic_num_mini_batch=1)
        vn = e.value_norm_state()
        info = e.happo_train(b, seed=3, use_factor=False, update_value_norm=False, **s)
        assert info.factor is None and e.value_norm_state() == vn
        assert [e.optim_state(a)["step"] for a in range(3)] == [5, 5, 5] and e.optim_state("critic")["step"] == 1
        for bad in (dict(actor_num_mini_batch=3), dict(critic_num_mini_batch=7)):
            with pytest.raises(ValueError, match="does not divide the batch's 20 steps"):
                e.happo_train(b, seed=3, **dict(s, **bad))
        with pytest.raises(ValueError, match="no seed and no indices"):
            e.happo_train(b, **s)
    finally:
        start(e, nets, csd)


# ---- 5. the fixture the reference wrote ------------------------------------------------------------------------------------------------------
def test_the_references_own_train_replayed_with_its_permutations():
    import torch as t
    from dc_rl_amd.engine import OnPolicyBatch
    from tests import actor_grad_ref as AG
    from tests import critic_grad_ref as GR
    from tests import optim_ref as O
    fx = TR.fixture()
    Tf, Nf, E, M = (int(fx[k]) for k in ("T", "N", "epochs", "num_mini_batch"))
    e = AR.engine(Nf, False)
    try:
        dev = e.device
        actor_sd = {k[len("actor_sd/"):]: v for k, v in fx.items() if k.startswith("actor_sd/")}
        critic_sd = {k[len("critic_sd/"):]: v for k, v in fx.items() if k.startswith("critic_sd/")}
        e.set_actor(0, dict(actor_sd, activation="tanh"))
        e.set_critic(critic_sd, None, "tanh")
        e.set_value_norm(dict(running_mean=0.0, running_mean_sq=0.0, debiasing_term=0.0))      # (a new ValueNorm)
        up = lambda x: t.from_numpy(np.ascontiguousarray(x)).to(dev)
        col0 = lambda x, dt: t.zeros((Tf, Nf, 3), dtype=dt, device=dev).index_copy_(2, t.tensor([0], device=dev), up(x).view(Tf, Nf, 1))
        obs = t.zeros((Tf, Nf, 3, 26), device=dev)
        obs[:, :, 0] = up(fx["obs"])
        adv = fx["advantages"].astype(np.float64)
        fields = dict.fromkeys(OnPolicyBatch.FIELDS)
        fields.update(obs=obs, actions=col0(fx["actions"], t.int32), action_log_probs=col0(fx["old_log_probs"], t.float32),
                      logits=t.zeros((Tf, Nf, 3, 3), device=dev), entropy=t.zeros((Tf, Nf, 3), device=dev), advantages=up(fx["advantages"]),
                      share_obs=up(fx["share_obs"]), values=t.zeros((Tf, Nf), device=dev), value_preds=up(fx["value_preds"]),
                      returns=up(fx["returns"]), adv_mean=t.tensor(adv.mean(), dtype=t.float64, device=dev),
                      adv_std=t.tensor(adv.std(), dtype=t.float64, device=dev))
        b = OnPolicyBatch(**fields)
        indices = {(0, ep): up(fx["actor_perms"][ep]) for ep in range(E)}
        indices.update({("critic", ep): up(fx["critic_perms"][ep]) for ep in range(E)})
        info = e.happo_train(b, indices=indices, ppo_epoch=E, critic_epoch=E, actor_num_mini_batch=M, critic_num_mini_batch=M, agent_order=(0,),
                             clip_param=float(fx["clip_param"]), entropy_coef=float(fx["entropy_coef"]), huber_delta=float(fx["huber_delta"]),
                             value_loss_coef=float(fx["value_loss_coef"]), lr=float(fx["lr"]), eps=float(fx["opti_eps"]),
                             weight_decay=float(fx["weight_decay"]), max_grad_norm=float(fx["max_grad_norm"]), beta=float(fx["beta"]))
        pa = O.sd_flat({k: v.numpy() for k, v in e.actor_state_dict(0).items()}, AG.FIELDS, AG.KEYS, AG.SHAPES)
        pc = O.sd_flat({k: v.numpy() for k, v in e.critic_state_dict().items()}, GR.FIELDS, GR.KEYS, GR.SHAPES)
        vn = e.value_norm_state()
        for who, p in (("actor", pa), ("critic", pc)):
            d = float(np.abs(p.astype(np.float64) - fx[who + "_p64"]).max())
            d32 = float(np.abs(fx[who + "_p32"].astype(np.float64) - fx[who + "_p64"]).max())
            print("%s after train(): %.3e from the reference's fp64 results, the reference's fp32 results %.3e: ratio %.2f" % (who, d, d32, d / d32))
            assert d32 > 0.0 and d <= TR.MARGIN * d32, who
        d = TR.scale_shift_distance((vn["scale"], vn["shift"]), fx["value_norm64"][-1])
        d32 = TR.scale_shift_distance(TR.derive(*fx["value_norm32"][-1]), fx["value_norm64"][-1])
        print("(scale, shift) after train(): %.3e from the reference's fp64 run, the reference's fp32 run %.3e: ratio %.2f" % (d, d32, d / d32))
        assert d32 > 0.0 and d <= TR.MARGIN * d32
        # the logged means are the reference's train_info (fp64 run), to what fp32 networks allow
        summ = info.summary()
        ref = dict(zip(("policy_loss", "dist_entropy", "actor_grad_norm", "ratio"), fx["actor_info64"]))
        for k, v in ref.items():
            assert summ["actor"][0][k] == pytest.approx(v, rel=1e-4, abs=1e-6), k
        assert summ["critic"]["value_loss"] == pytest.approx(fx["critic_info64"][0], rel=1e-4)
        assert summ["critic"]["critic_grad_norm"] == pytest.approx(fx["critic_info64"][1], rel=1e-4)
    finally:
        e.close()


# ---- 6. the loop never waits; copies; refusals ------------------------------------------------------------------------------------------------
def test_collect_train_collect_never_waits_for_the_host(rig):
    import torch
    e, nets, csd, _ = rig
    try:
        e.reset()
        s = dict(SCHEDULE, critic_num_mini_batch=2)
        warm = e.collect(T)
        e.happo_train(warm, seed=1, **s)      # (the handle's buffers are allocated on their first use)
        start(e, nets, csd)
        e.reset()
        torch.cuda.synchronize(e.device)
        torch.cuda.set_sync_debug_mode("error")
        try:
            b = e.collect(T)
            info = e.happo_train(b, seed=9, **s)
            b2 = e.collect(T)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize(e.device)
        summ = info.summary()
        assert np.isfinite(summ["critic"]["value_loss"]) and bool(torch.isfinite(b2.returns).all())
        assert [e.optim_state(a)["step"] for a in range(3)] == [4, 4, 4] and e.optim_state("critic")["step"] == 4
        assert e.value_norm_state()["debiasing_term"] != VN0["debiasing_term"]
        assert not torch.equal(b.logits, b2.logits)
    finally:
        start(e, nets, csd)
        e.reset()


def test_a_deep_copy_trains_on_and_agrees(rig):
    from tests.test_gpu_actor_stats import _vec
    _, nets, csd, _ = rig
    v = _vec(N)
    try:
        for a in range(3):
            v.set_actor(a, nets[a].state_dict())
        v.set_critic(csd, CR.VALUE_NORM)
        v.set_value_norm(VN0)
        v.reset()      # (behind the actors: the closed loop's first actions are chosen from the reset's observations)
        s = dict(SCHEDULE, critic_num_mini_batch=2)
        v.happo_train(v.collect(T), seed=4, **s)
        c = copy.deepcopy(v)
        try:
            assert c.engine._value_norm_installed and c.value_norm_state() == v.value_norm_state()
            assert "value_norm" in v.optim_state("critic") and "value_norm" not in v.optim_state(0)
            for w in (v, c):
                w.happo_train(w.collect(T), seed=5, **s)
            assert_same_state(training_state(v.engine), training_state(c.engine), "deep copy")
            assert v.value_norm_state() == c.value_norm_state() and v.optim_state("critic")["step"] == 8
        finally:
            c.close()
    finally:
        v.close()


def test_every_refusal_reaches_python_and_training_state_stays(rig):
    import torch
    e, nets, csd, b = rig
    dev = e.device
    before = training_state(e)
    idx = e.permutation(T * N, 1, 0)
    p = lambda x: C.c_void_p(x.data_ptr())
    seg = (L.SdcGatherSegment * 1)()
    dst = torch.zeros((T * N, 29), device=dev)
    seg[0].src, seg[0].dst, seg[0].src_stride, seg[0].dst_stride, seg[0].n_dwords = b.share_obs.data_ptr(), dst.data_ptr(), 29, 29, 29
    gather = lambda **kw: e._call(e.lib.sdc_gather_rows, kw.get("idx", p(idx)), kw.get("n_rows", 800), kw.get("n_src", 800), seg,
                                  kw.get("n_segs", 1), kw.get("bad", None), e._stream(), refuses=True)
    cases = [
        (r"permutation: n = 0 outside", lambda: e.permutation(0, 1)),
        (r"permutation: n = 2147483648 outside", lambda: e.permutation(2 ** 31, 1)),
        (r"sdc_permutation: n = 0 outside \[1, 2147483647\]", lambda: e._call(e.lib.sdc_permutation, 0, 1, 0, p(idx), e._stream(), refuses=True)),
        ("sdc_permutation: null perm", lambda: e._call(e.lib.sdc_permutation, 8, 1, 0, None, e._stream(), refuses=True)),
        ("sdc_permutation: perm not dword-aligned",
         lambda: e._call(e.lib.sdc_permutation, 8, 1, 0, C.c_void_p(idx.data_ptr() + 2), e._stream(), refuses=True)),
        ("sdc_gather_rows: n_rows = 0 must be positive", lambda: gather(n_rows=0)),
        (r"sdc_gather_rows: n_src_rows = 0 outside", lambda: gather(n_src=0)),
        ("sdc_gather_rows: null idx or segs", lambda: gather(idx=None)),
        ("sdc_gather_rows: idx / bad not dword-aligned", lambda: gather(bad=C.c_void_p(idx.data_ptr() + 1))),
        (r"sdc_gather_rows: n_segs = 17 outside \[1, 16\]", lambda: gather(n_segs=17)),
        ("minibatch: len\\(indices\\) = 100 is not a positive multiple of n_envs = 40", lambda: e.minibatch(b, idx[:100])),
        ("minibatch: indices must be a contiguous int32 CUDA tensor", lambda: e.minibatch(b, idx.long())),
        ("minibatch: indices must be a contiguous int32 CUDA tensor", lambda: e.minibatch(b, idx[:0])),
        ("minibatch: agent = 3 must be 0", lambda: e.minibatch(b, idx, agent=3)),
        ("minibatch: neither the actors' nor the critic's", lambda: e.minibatch(b, idx, critic=False, actors=False)),
        ("minibatch: into must be a MiniBatch of 20 steps", lambda: e.minibatch(b, idx, into=e.minibatch(b, idx[:400]))),
        ("minibatch: factor must be a contiguous float32 CUDA tensor", lambda: e.minibatch(b, idx, factor=torch.ones(T, device=dev))),
        (r"sdc_value_norm_update: beta = 1.000000 outside \[0, 1\)", lambda: e.value_norm_update(b.returns, 1.0)),
        (r"sdc_value_norm_update: beta = -0.100000 outside", lambda: e.value_norm_update(b.returns, -0.1)),
        ("sdc_value_norm_update: n = 0 must be positive", lambda: e.value_norm_update(b.returns[:0])),
        ("value_norm_update: returns must be a contiguous float32 CUDA tensor", lambda: e.value_norm_update(b.returns.double())),
        ("sdc_set_value_norm: an entry that is not finite", lambda: e.set_value_norm(dict(VN0, running_mean=float("nan")))),
        ("sdc_set_value_norm: running_mean_sq and debiasing_term must not be negative", lambda: e.set_value_norm(dict(VN0, debiasing_term=-1.0))),
        ("sdc_value_loss_normed: clip_param = -1.000000 must be finite and not negative",
         lambda: e.value_loss(b.returns, b.returns, b.returns, clip_param=-1.0)),
        ("happo_train: num_mini_batch = 3 does not divide", lambda: e.happo_train(b, seed=1, lr=LR, actor_num_mini_batch=3)),
        ("happo_train: agents = \\(0, 0\\) must name", lambda: e.happo_train(b, seed=1, lr=LR, agent_order=(0, 0))),
        (r"happo_train: indices\[\(0, 0\)\] must be a contiguous int32 CUDA tensor", lambda: e.happo_train(b, lr=LR, indices={(0, 0): idx[:400]})),
    ]
    for match, call in cases:
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(KeyError, match="running_mean"):
        e.set_value_norm(dict(mean=1.0))
    fresh = AR.engine(N, False)
    try:
        for match, call in (("sdc_set_value_norm: sdc_set_critic first", lambda: fresh.set_value_norm(VN0)),
                            ("sdc_get_value_norm: sdc_set_critic first", lambda: fresh.value_norm_state()),
                            ("sdc_value_norm_update: sdc_set_critic first", lambda: fresh.value_norm_update(b.returns.to(fresh.device)))):
            with pytest.raises(ValueError, match=match):
                call()
        fresh.set_critic(csd, CR.VALUE_NORM)
        with pytest.raises(ValueError, match="sdc_get_value_norm: no ValueNorm is installed"):
            fresh.value_norm_state()
        # set_critic and set_critic_value_norm uninstall
        fresh.set_value_norm(VN0)
        fresh.set_critic_value_norm((0.5, 4.0))
        assert not fresh._value_norm_installed
        with pytest.raises(ValueError, match="no ValueNorm is installed"):
            fresh.value_norm_update(b.returns.to(fresh.device))
        fresh.set_value_norm(VN0)
        fresh.set_critic(csd, CR.VALUE_NORM)
        with pytest.raises(ValueError, match="no ValueNorm is installed"):
            fresh.value_norm_state()
    finally:
        fresh.close()
    assert not bool(dst.any())      # (no refused gather wrote a row)
    assert_same_state(training_state(e), before, "after the refusals")
