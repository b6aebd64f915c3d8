"""The on-policy batch on the device (sdc_gae, sdc_action_log_probs, SdcEngine.collect; csrc/sdc_onpolicy.hip) held to the NumPy
restatement tests/onpolicy_ref.py -- which tests/test_onpolicy_ref.py holds to the reference's compute_returns bit for bit -- and to the
header's contract (include/sustaindc_hip.h THE ON-POLICY BATCH):

 1. sdc_gae, EVERY OUTPUT BIT (returns, advantages, masks, value_preds) against the restatement: N in {1, 63, 64, 65, 130} x T in
    {1, 2, U-1, U, U+1, 37} (U = SDC_STATS_UNROLL) x six done patterns, and over them the three (gamma, lambda) pairs x use_gae x
    reward_agent x first_done null / given x values of magnitude 1e-3 / 1e3; every output sits between guard rows of a NaN pattern in
    ONE allocation (so a neighbour's row 0 is its neighbour's guard) that must come back untouched; moments within 1e-12 relative of
    the restatement's (both sum the same fp32 advantages in fp64);  2. the fixture's inputs give the reference's returns bit for bit;
 3. two runs give the same bits, and so does a pinned non-default stream;  4. sdc_action_log_probs against the restatement: at most
    1 fp32 ulp, at most 1 result in 1000 different at all (the device's fp64 exp / log may differ from libm's in the last place),
    logits of scale 2.5 with entries at +-80; summed over a chunk it agrees with sdc_rollout_actor_stats' LOGP and ENTROPY under that
    test's own bar plus the fp32 roundings;  5. collect against a twin engine stepping with rollout_actor in the same segments, inside
    one episode and across an auto-reset, chained through last_done, the engine left where the twin is;  6. the refusals.

The engines of 1-4 are never reset: both calls are pure functions of their arrays."""
import re

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import actor_ref as AR
from tests import critic_ref as CR
from tests import onpolicy_ref as R
from tests.plan_util import refused

pytestmark = pytest.mark.gpu

UNROLL = int(re.search(r"#define SDC_STATS_UNROLL (\d+)", open(L.CSRC + "/sdc_stats.hpp").read()).group(1))
NS = (1, 63, 64, 65, 130)
TS = (1, 2, UNROLL - 1, UNROLL, UNROLL + 1, 37)
REL = 1e-12
SCALE, SHIFT = float(np.sqrt(CR.VALUE_NORM[1])), float(CR.VALUE_NORM[0])
EP = 48


@pytest.fixture(scope="module")
def engines():
    """{N: an engine of N envs with a critic (for its scale and shift), never reset}, built on first use"""
    from dc_rl_amd.engine import SdcEngine
    made = {}

    def get(N):
        if N not in made:
            made[N] = SdcEngine(N, episode_steps=EP, hist_cap=128)
            made[N].set_critic(CR.make_critic(3), CR.VALUE_NORM)
        return made[N]

    yield get
    for e in made.values():
        e.close()


def _guarded(torch, rows, N, device):
    """one fp32 allocation holding arrays of `rows` rows of N, a guard row in front of each and one behind the last, all of it the
    NaN pattern -> (the flat tensor, [the arrays' views], a boolean mask of the guard entries)"""
    total = sum(rows) * N + (len(rows) + 1) * N
    flat = torch.full((total,), R.NAN_BITS, dtype=torch.int32, device=device).view(torch.float32)
    guard = np.ones(total, dtype=bool)
    views, o = [], N
    for r in rows:
        views.append(flat[o:o + r * N].view(r, N))
        guard[o:o + r * N] = False
        o += (r + 1) * N
    return flat, views, guard


def _gae(eng, rew, done, values, gamma, lam, use_gae=1, agent=0, first=None, preds=True):
    """sdc_gae through the library with guarded outputs -> {name: NumPy array}; the guards checked"""
    import torch
    t, dev, N = torch, eng.device, eng.n_envs
    T = done.shape[0]
    d_rew, d_done, d_val = (t.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (rew, done, values))
    d_first = None if first is None else t.from_numpy(first).to(dev)
    flat, (ret, adv, masks, vp), guard = _guarded(t, (T, T, T + 1, T + 1), N, dev)
    mom = t.full((6,), float("nan"), dtype=t.float64, device=dev)
    p = lambda x: None if x is None else x.data_ptr()
    eng._behind_torch_stream()
    eng._call(eng.lib.sdc_gae, T, p(d_rew), agent, p(d_done), p(d_first), p(d_val), gamma, lam, use_gae, p(ret), p(adv), p(masks),
              p(vp) if preds else None, mom.data_ptr() + 16, eng._stream(), refuses=True)
    t.cuda.synchronize()
    raw = flat.view(t.int32).cpu().numpy()
    assert (raw[guard] == R.NAN_BITS).all(), ("a guard row was written", N, T, int((raw[guard] != R.NAN_BITS).sum()))
    if not preds:
        assert (vp.view(t.int32).cpu().numpy() == R.NAN_BITS).all()
    m = mom.cpu().numpy()
    assert np.isnan(m[[0, 1, 4, 5]]).all()
    return dict(returns=ret.cpu().numpy(), advantages=adv.cpu().numpy(), masks=masks.cpu().numpy(), value_preds=vp.cpu().numpy(),
                moments=m[2:4])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_gae(got, rew, done, values, gamma, lam, use_gae, agent, first, what):
    """-> the moments' largest relative difference"""
    ret, adv, masks = R.gae(rew, done, values, gamma, lam, bool(use_gae), agent, first)
    want = dict(returns=ret, advantages=adv, masks=masks, value_preds=R.value_preds(values, np.float32(SCALE), np.float32(SHIFT)))
    for k, w in want.items():
        if not np.array_equal(_bits(got[k]), _bits(w)):
            bad = np.argwhere(_bits(got[k]) != _bits(w))
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], w[tuple(bad[0])]))
    mean, std = R.moments(adv)
    rel = max(abs(got["moments"][0] - mean) / abs(mean), abs(got["moments"][1] - std) / std if std > 0 else abs(got["moments"][1]))
    assert rel <= REL, (what, "moments", got["moments"], (mean, std), rel)
    return rel


@pytest.mark.parametrize("N", NS)
def test_gae_every_output_bit(engines, N):
    eng = engines(N)
    worst, calls = 0.0, 0
    for ti, T in enumerate(TS):
        for pi, pattern in enumerate(R.DONE_PATTERNS):
            done = R.done_pattern(pattern, T, N)
            # six variants: every (gamma, lambda) pair with use_gae off and on; the other switches rotate with the shape and the pattern
            # so that each of their values meets every T, every pattern and both use_gae
            for v in range(6):
                gamma, lam = R.GAMMA_LAMBDA[v % 3]
                use_gae, agent = v % 2, (v + ti + pi) % 3
                magnitude = (1e-3, 1e3)[(v // 2 + ti + pi) % 2]
                first = ((np.arange(N) + v) % 3 == 0).astype(np.uint8) if (v // 3 + pi) % 2 else None
                rew, values = R.inputs(T, N, 1000 * ti + 10 * pi + v, magnitude)
                got = _gae(eng, rew, done, values, gamma, lam, use_gae, agent, first)
                worst = max(worst, _assert_gae(got, rew, done, values, gamma, lam, use_gae, agent, first,
                                               (N, T, pattern, gamma, lam, use_gae, agent, magnitude, first is not None)))
                calls += 1
    assert calls == 216
    print("sdc_gae at N = %d: %d calls, every output bit; moments against the restatement: max relative difference %.2e" % (N, calls, worst))


def test_gae_every_switch_meets_every_other(engines):
    """the full product of the switches at one shape (N = 65, T = UNROLL + 1, envs done at different steps)"""
    N, T = 65, UNROLL + 1
    eng, done = engines(N), R.done_pattern("staggered", UNROLL + 1, 65)
    first = (np.arange(N) % 2).astype(np.uint8)
    n = 0
    for gamma, lam in R.GAMMA_LAMBDA:
        for use_gae in (0, 1):
            for agent in (0, 1, 2):
                for fd in (None, first):
                    for magnitude in (1e-3, 1e3):
                        rew, values = R.inputs(T, N, n, magnitude)
                        got = _gae(eng, rew, done, values, gamma, lam, use_gae, agent, fd)
                        _assert_gae(got, rew, done, values, gamma, lam, use_gae, agent, fd, (gamma, lam, use_gae, agent, magnitude))
                        n += 1
    assert n == 72


def test_gae_without_value_preds_and_without_moments(engines):
    import torch
    eng = engines(65)
    rew, values = R.inputs(9, 65, 4)
    done = R.done_pattern("consecutive", 9, 65)
    got = _gae(eng, rew, done, values, 0.99, 0.95, preds=False)      # (value_preds untouched: checked inside)
    ret, adv, masks = R.gae(rew, done, values, 0.99, 0.95)
    assert np.array_equal(_bits(got["returns"]), _bits(ret)) and np.array_equal(_bits(got["masks"]), _bits(masks))
    # the binding: moments and value_preds only when asked for, the same bits as the raw call
    dev = eng.device
    args = [torch.from_numpy(x).to(dev) for x in (rew, done, values)]
    res = eng.gae(*args, 0.99, 0.95, want_moments=False)
    assert res.moments is None and res.value_preds is None
    assert np.array_equal(_bits(res.returns.cpu().numpy()), _bits(ret)) and np.array_equal(_bits(res.advantages.cpu().numpy()), _bits(adv))
    full = eng.gae(*args, 0.99, 0.95, want_value_preds=True)
    assert full.moments.dtype == torch.float64 and full.moments.shape == (2,) and full.value_preds.shape == (10, 65)
    assert np.array_equal(full.moments.cpu().numpy(), got["moments"])


def test_gae_gives_the_references_returns_on_the_fixture(engines):
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "onpolicy", "onpolicy_returns.npz")) as f:
        fx = {k: f[k] for k in f.files}
    T, N = fx["done"].shape
    eng = engines(N)
    rew = np.zeros((T, N, 3), dtype=np.float32)
    rew[..., 0] = fx["rew"]
    for i, (gamma, lam) in enumerate(R.GAMMA_LAMBDA):
        for use_gae in (0, 1):
            got = _gae(eng, rew, fx["done"], fx["values"], gamma, lam, use_gae)
            assert np.array_equal(_bits(got["returns"]), _bits(fx[f"plain_returns_{i}_{use_gae}"])), (gamma, lam, use_gae)
    gamma, lam = R.GAMMA_LAMBDA[0]
    got = _gae(eng, rew, fx["done"], fx["norm_values"], gamma, lam, 1)
    assert np.array_equal(_bits(got["returns"]), _bits(fx["norm_returns"]))


def test_gae_twice_and_on_a_pinned_stream(engines):
    import torch
    eng = engines(130)
    rew, values = R.inputs(37, 130, 8, 1e3)
    done = R.done_pattern("staggered", 37, 130)
    first = (np.arange(130) % 5 == 0).astype(np.uint8)
    run = lambda: _gae(eng, rew, done, values, 0.99, 0.95, 1, 1, first)
    a, b = run(), run()
    eng.use_stream(torch.cuda.Stream(device=eng.device))
    try:
        c = run()
    finally:
        eng.use_stream(None)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


# ---- sdc_action_log_probs ------------------------------------------------------------------------------------------------------------
def _logits(T, N, seed):
    """logits [T, N, 3, 3] of scale 2.5, every 17th (step, env, agent) with one logit at +80 or -80; actions [T, N, 3]"""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((T, N, 3, 3)) * 2.5).astype(np.float32)
    flat = logits.reshape(-1, 3)
    k = np.arange(0, flat.shape[0], 17)
    flat[k, k % 3] = np.where(k % 2 == 0, np.float32(80.0), np.float32(-80.0))
    actions = rng.integers(0, 3, (T, N, 3)).astype(np.int32)
    return actions, logits


@pytest.mark.parametrize("N", NS)
def test_action_log_probs_against_the_restatement(engines, N):
    """(the restatement itself, evaluated in long double against fp64 on these inputs, moves no rounded result: printed below)"""
    import torch
    eng = engines(N)
    n = differ = differ_ent = own = 0
    for T in TS:
        actions, logits = _logits(T, N, 100 * N + T)
        want_lp, want_ent = R.action_log_probs(actions, logits)
        lp80, ent80 = R.action_log_probs(actions, logits, np.longdouble)
        own += int((R.ulps(want_lp, lp80) > 0).sum() + (R.ulps(want_ent, ent80) > 0).sum())
        a, l = torch.from_numpy(actions).to(eng.device), torch.from_numpy(logits).to(eng.device)
        lp, ent = eng.action_log_probs(a, l)
        assert lp.shape == ent.shape == (T, N, 3) and lp.dtype == ent.dtype == torch.float32
        only, none = eng.action_log_probs(a, l, want_entropy=False)
        assert none is None and torch.equal(only.view(torch.int32), lp.view(torch.int32))
        u_lp, u_ent = R.ulps(lp.cpu().numpy(), want_lp), R.ulps(ent.cpu().numpy(), want_ent)
        assert u_lp.max() <= 1 and u_ent.max() <= 1, (N, T, int(u_lp.max()), int(u_ent.max()))
        n += u_lp.size
        differ += int((u_lp > 0).sum())
        differ_ent += int((u_ent > 0).sum())
    print("sdc_action_log_probs at N = %d: %d results each; different from the restatement (all by 1 ulp): %d log-probs, %d entropies; "
          "fp64 against long double in the restatement itself: %d" % (N, n, differ, differ_ent, own))
    assert own * 1000 <= 2 * n, "choose other seeds: fp64 itself moves more than 1 result in 1000 on these inputs"
    assert differ * 1000 <= max(n, 1000) and differ_ent * 1000 <= max(n, 1000), (N, n, differ, differ_ent)


# ---- the closed loop: collect --------------------------------------------------------------------------------------------------------
N_COLLECT = 130


def _actor_engine():
    e = AR.engine(N_COLLECT, False, steps=EP)
    AR.set_actors(e, [AR.torch_actor(300 + a) for a in range(3)])
    e.set_critic(CR.make_critic(21), CR.VALUE_NORM)
    e.reset()
    return e


@pytest.fixture(scope="module")
def trio():
    """three engines with one seed, the actors and the critic set, just reset: for collect, its twin and the chained calls"""
    engs = [_actor_engine() for _ in range(3)]
    yield engs
    for e in engs:
        e.close()


def _same(a, b, what):
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    v = torch.int32 if a.dtype == torch.float32 else a.dtype
    assert torch.equal(a.contiguous().view(v), b.contiguous().view(v)), what


def _twin_collect(eng, T):
    """T steps on the twin with rollout_actor in collect's segments -> the per-step fields as collect lays them out"""
    import torch
    obs, share = [eng.obs.clone()[None]], [eng.share_obs.clone()[None]]
    values = [eng.critic_values(eng.share_obs.clone())[None]]
    rew, done, acts, logits = [], [], [], []
    k = 0
    while k < T:
        K = min(T - k, eng.steps_to_episode_end())
        o, s, r, d, _, a, l, v = eng.rollout_actor(K, sample=True, want_logits=True, want_values=True)
        for lst, x in ((obs, o), (share, s), (rew, r), (done, d), (acts, a), (logits, l), (values, v)):
            lst.append(x)
        k += K
    cat = lambda xs: torch.cat(xs, 0)
    return dict(obs=cat(obs), share_obs=cat(share), rewards=cat(rew), dones=cat(done), actions=cat(acts), logits=cat(logits), values=cat(values))


def _assert_batch(b, twin, T, gamma, lam, first=None):
    import torch
    N = N_COLLECT
    for k, x in twin.items():
        _same(getattr(b, k), x, k)
    assert b.obs.shape == (T + 1, N, 3, 26) and b.share_obs.shape == (T + 1, N, 29) and b.values.shape == (T + 1, N)
    rew, done, values = (getattr(b, k).cpu().numpy() for k in ("rewards", "dones", "values"))
    ret, adv, masks = R.gae(rew, done, values, gamma, lam, True, 0, None if first is None else first.cpu().numpy())
    for k, w in (("returns", ret), ("advantages", adv), ("masks", masks)):
        assert np.array_equal(_bits(getattr(b, k).cpu().numpy()), _bits(w)), k
    mean, std = R.moments(adv)
    assert b.adv_mean.dim() == 0 and b.adv_mean.dtype == torch.float64 and b.adv_std.dim() == 0
    assert abs(float(b.adv_mean) - mean) <= REL * abs(mean) and abs(float(b.adv_std) - std) <= REL * std
    lp, ent = R.action_log_probs(b.actions.cpu().numpy(), b.logits.cpu().numpy())
    assert R.ulps(b.action_log_probs.cpu().numpy(), lp).max() <= 1 and R.ulps(b.entropy.cpu().numpy(), ent).max() <= 1
    # value_preds * scale + shift returns to values within 2 ulp
    vp = b.value_preds.cpu().numpy()
    assert np.array_equal(_bits(vp), _bits(R.value_preds(values, np.float32(SCALE), np.float32(SHIFT))))
    back = vp * np.float32(SCALE) + np.float32(SHIFT)
    u = int(R.ulps(back, values).max())
    print("value_preds * scale + shift against values: at most %d ulp" % u)
    assert u <= 2
    _same(b.last_done, b.dones[T - 1], "last_done")
    want = (b.advantages.double() - b.adv_mean) / (b.adv_std + 1e-5)
    na = b.normalized_advantages()
    assert na.dtype == torch.float32 and na.shape == (T, N) and float((na.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    flat = b.flat()
    assert flat["obs"].shape == (T * N, 3, 26) and flat["returns"].shape == (T * N,) and flat["masks"].shape == (T * N,)
    _same(flat["values"], b.values[:T].reshape(-1), "flat values")
    assert flat["actions"].data_ptr() == b.actions.data_ptr()      # (views)


def test_collect_inside_an_episode_across_a_reset_and_chained(trio):
    import torch
    from tests.test_gpu_mark import _grab
    a, twin, chained = trio
    # 20 steps inside the first episode
    b = a.collect(20)
    _assert_batch(b, _twin_collect(twin, 20), 20, 0.99, 0.95)
    assert not bool(b.dones.any()) and bool((b.masks == 1).all()) and a.steps_to_episode_end() == EP - 20
    # 60 steps from step 20: across the auto-reset behind step 47 (index 27 of this batch)
    first = b.last_done
    b60 = a.collect(60, gamma=0.9, gae_lambda=0.0, first_done=first)
    t60 = _twin_collect(twin, 60)
    _assert_batch(b60, t60, 60, 0.9, 0.0, first)
    end = EP - 20 - 1
    assert bool(b60.dones[end].all()) and int(b60.dones.sum()) == N_COLLECT and bool((b60.masks[end + 1] == 0).all())
    assert float(b60.masks.sum()) == 61 * N_COLLECT - N_COLLECT
    # the row after the done step is the new episode's observation: the twin's engine held it after its first segment, and it is not
    # the old episode's next row (the step counter in share_obs starts again)
    assert not torch.equal(b60.share_obs[end + 1], b60.share_obs[end])
    # the engine is left where the twin is
    ga, gt = _grab(a), _grab(twin)
    for k in ga:
        assert np.array_equal(ga[k], gt[k]), k
    for nm in ("obs", "share_obs", "rew", "done"):
        _same(getattr(a, nm), getattr(twin, nm), nm)
    assert a.steps_to_episode_end() == twin.steps_to_episode_end() == EP - (80 - EP)
    # two calls chained through last_done equal one call of the summed length in every per-step field (not the returns: they
    # depend on the bootstrap)
    c0 = chained.collect(20)
    c1 = chained.collect(25, gamma=0.9, gae_lambda=0.0, first_done=c0.last_done)
    c2 = chained.collect(35, gamma=0.9, gae_lambda=0.0, first_done=c1.last_done)
    for k in ("obs", "share_obs", "masks", "values", "value_preds"):
        _same(torch.cat([getattr(c1, k)[:25], getattr(c2, k)]), getattr(b60, k), k)
        _same(getattr(c1, k)[25], getattr(c2, k)[0], k + " hand-over")
    for k in ("actions", "logits", "action_log_probs", "entropy", "rewards", "dones"):
        _same(torch.cat([getattr(c1, k), getattr(c2, k)]), getattr(b60, k), k)
    _same(c2.last_done, b60.last_done, "last_done")


def test_log_prob_sums_agree_with_rollout_actor_stats(trio):
    """sum_k log_probs over a chunk against sdc_rollout_actor_stats' LOGP (and ENTROPY) on a twin: that test's bar, REL of the summed
    |terms|, plus the fp32 roundings of the K terms (half an ulp each; a whole one allowed for)"""
    import torch
    a, twin, _ = trio
    K = min(16, a.steps_to_episode_end())
    assert K >= 4 and a.steps_to_episode_end() == twin.steps_to_episode_end()
    st = twin.rollout_actor_stats(K, sample=True)
    out = a.rollout_actor(K, sample=True, want_logits=True)
    lp, ent = a.action_log_probs(out[5], out[6])
    for got, want, name in ((lp, st.policy.sums[..., L.POLICY_LOGP], "LOGP"), (ent, st.policy.sums[..., L.POLICY_ENTROPY], "ENTROPY")):
        g = got.cpu().numpy().astype(np.float64)
        bound = REL * np.abs(g).sum(0) + np.spacing(np.abs(got.cpu().numpy())).astype(np.float64).sum(0)
        err = np.abs(g.sum(0) - want.cpu().numpy())
        print("%s over %d steps: max |sum - stats| %.3e, bound there %.3e" % (name, K, err.max(), bound[np.unravel_index(err.argmax(), err.shape)]))
        assert (err <= bound).all(), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_untouched(trio):
    import torch
    a = trio[0]
    N, dev = N_COLLECT, a.device
    T = 3
    rew = torch.zeros((T, N, 3), device=dev)
    done = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    values = torch.zeros((T + 1, N), device=dev)
    acts = torch.zeros((T, N, 3), dtype=torch.int32, device=dev)
    logits = torch.zeros((T, N, 3, 3), device=dev)
    for bad in (1.5, -0.1, float("nan"), float("inf")):
        refused(a, "gamma = .* outside \\[0, 1\\]", lambda: a.gae(rew, done, values, gamma=bad))
        refused(a, "gae_lambda = .* outside \\[0, 1\\]", lambda: a.gae(rew, done, values, gae_lambda=bad))
    refused(a, "reward_agent = 3 outside \\[0, 2\\]", lambda: a.gae(rew, done, values, reward_agent=3))
    refused(a, "reward_agent = -1 outside", lambda: a.gae(rew, done, values, reward_agent=-1))
    refused(a, "use_gae = 2 outside \\{0, 1\\}", lambda: a.gae(rew, done, values, use_gae=2))
    refused(a, "gae: rew must be a contiguous float32 CUDA tensor of shape \\(T, n_envs, 3\\)", lambda: a.gae(rew[:, :-1], done, values))
    refused(a, "gae: done must be", lambda: a.gae(rew, done.to(torch.float32), values))
    refused(a, "gae: values must be .* \\(T \\+ 1, n_envs\\)", lambda: a.gae(rew, done, values[:T]))
    refused(a, "gae: first_done must be", lambda: a.gae(rew, done, values, first_done=done))
    refused(a, "gae: rew must be", lambda: a.gae(rew.cpu(), done, values))
    refused(a, "action_log_probs: actions must be", lambda: a.action_log_probs(acts.long(), logits))
    refused(a, "action_log_probs: logits must be .* \\(T, n_envs, 3, 3\\)", lambda: a.action_log_probs(acts, logits[:-1]))
    refused(a, "action_log_probs: actions must be", lambda: a.action_log_probs(acts[:0], logits[:0]))
    # what only the library sees: the raw calls
    p = lambda x: x.data_ptr()
    raw = lambda **kw: a._call(a.lib.sdc_gae, kw.get("T", T), kw.get("rew", p(rew)), 0, p(done), None, p(values), 0.99, 0.95, 1,
                               kw.get("ret", p(values)), p(values), p(values), None, kw.get("mom"), a._stream(), refuses=True)
    refused(a, "sdc_gae: n_steps = 0 must be positive", lambda: raw(T=0))
    refused(a, "sdc_gae: null array", lambda: raw(rew=None))
    refused(a, "sdc_gae: null array", lambda: raw(ret=None))
    refused(a, "not dword-aligned", lambda: raw(rew=p(rew) + 2))
    refused(a, "sdc_gae: moments not 16-byte aligned", lambda: raw(mom=p(values) + 8))
    rawl = lambda **kw: a._call(a.lib.sdc_action_log_probs, kw.get("T", T), kw.get("acts", p(acts)), p(logits), kw.get("lp", p(rew)),
                                kw.get("ent"), a._stream(), refuses=True)
    refused(a, "sdc_action_log_probs: n_steps = -1 must be positive", lambda: rawl(T=-1))
    refused(a, "sdc_action_log_probs: null array", lambda: rawl(acts=None))
    refused(a, "sdc_action_log_probs: null array", lambda: rawl(lp=None))
    refused(a, "sdc_action_log_probs: .* not dword-aligned", lambda: rawl(ent=p(values) + 1))
    # collect
    refused(a, "collect: n_steps = 0 must be positive", lambda: a.collect(0))
    refused(a, "collect: first_done must be", lambda: a.collect(4, first_done=done))


def test_collect_and_value_preds_refused_without_a_critic_an_actor_or_a_reset():
    import torch
    bare = AR.engine(N_COLLECT, False, steps=EP)
    bare.reset()
    try:
        refused(bare, "collect: set_actor all three agents first", lambda: bare.collect(4))
        AR.set_actors(bare, [AR.torch_actor(300 + a) for a in range(3)])
        refused(bare, "collect: set_critic first", lambda: bare.collect(4))
        dev = bare.device
        rew = torch.zeros((2, N_COLLECT, 3), device=dev)
        done = torch.zeros((2, N_COLLECT), dtype=torch.uint8, device=dev)
        values = torch.zeros((3, N_COLLECT), device=dev)
        refused(bare, "sdc_gae: value_preds asked for while no critic is set", lambda: bare.gae(rew, done, values, want_value_preds=True))
        assert bare.gae(rew, done, values).value_preds is None      # (without them the call needs no critic)
    finally:
        bare.close()
    fresh = AR.engine(N_COLLECT, False, steps=EP)
    try:
        AR.set_actors(fresh, [AR.torch_actor(300 + a) for a in range(3)])
        fresh.set_critic(CR.make_critic(21), CR.VALUE_NORM)
        with pytest.raises(ValueError, match="collect: no episode is running: call reset\\(\\) first"):
            fresh.collect(4)
        assert fresh.steps_to_episode_end() == 0
    finally:
        fresh.close()
