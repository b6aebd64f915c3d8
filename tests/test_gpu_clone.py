"""Forking envs on the device (SdcEngine.clone_envs over sdc_clone_envs): env dst[k] becomes a copy of env src[k].

1. On every step mapping (pair, quad, wide, wide_gen, and the general kernel of a staggered batch), full rings, requests in flight:
   a clone is its source bit for bit -- every output row on every step to the episode end under the same actions, every state
   field just before the boundary -- and a lock-step batch keeps the kernel it ran before the clone.
2. Divergent branches: cloned oracles, different actions, the fp64 oracle every step through the auto-reset, whose draws are
   held to dst's OWN global index (verify mode on: the verify kernel checks dst's reward state every step).
3. The ring's slot-major mirror (49 152 envs, contiguous and scattered dst) and a rollout() after a clone.
4. The closed loop: rollout_actor right after a clone (the library's copy of the latest observations follows).
5. The refusals, each of which leaves the state untouched."""
import ctypes as C

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import SustainDCVecEnv, dc_config, traces
from dc_rl_amd.engine import SdcEngine, _CHECKPOINT, _STATE_DTYPES
from oracle import pyoracle as po
from tests import gpu_helpers as G
from tests.production_rig import ProductionRig, sample_parts

pytestmark = pytest.mark.gpu

EP = 48          # episode_steps: the clone at CLONE_AT, then to the boundary
CLONE_AT = 24
RSV = L.INFO_IDX["reserved"]


def _acts(N, g):
    import torch
    return torch.randint(0, 3, (N, 3), dtype=torch.int32, generator=g).cuda()


def _pending_envs(eng):
    return np.nonzero((eng.get_state("header")[:, G.hdr_pend()] != 0).any(axis=1))[0]


def _pick_pairs(eng, geom, rng, n_pairs=64):
    """(src, dst) with the envs of the first and last workgroups on both sides, a src and a dst with a re-centring request in
    flight, a src with tasks queued, the rest random; no env twice, no dst a src."""
    N = eng.n_envs
    parts = sample_parts(N, geom)
    first, last = parts["first"], parts["last"]
    pend = _pending_envs(eng)
    queued = np.nonzero(eng.info[:, L.INFO_IDX["ls_tasks_in_queue"]].cpu().numpy() > 0)[0]
    assert len(pend) >= 2 and len(queued) >= 1, (len(pend), len(queued))
    used, src, dst = set(), [], []

    def take(pool, out, k):
        for e in pool:
            if k == 0:
                break
            if int(e) not in used:
                used.add(int(e))
                out.append(int(e))
                k -= 1

    take(first[:2], src, 2)
    take(first[-2:], dst, 2)
    take(last[:2], src, 2)
    take(last[-2:], dst, 2)
    pend_p = rng.permutation(pend)          # (often only a few: one for each side first)
    take(pend_p, src, 1)
    take(pend_p, dst, 1)
    take(pend_p, src, 1)
    take(pend_p, dst, 1)
    take(rng.permutation(queued), src, 2)
    rest = [e for e in rng.permutation(N) if int(e) not in used]
    while len(src) < n_pairs:
        take(rest[:1], src, 1)
        rest = rest[1:]
    while len(dst) < n_pairs:
        take(rest[:1], dst, 1)
        rest = rest[1:]
    s, d = np.array(src[:n_pairs]), np.array(dst[:n_pairs])
    assert set(s).isdisjoint(d) and len(set(d)) == len(d)
    assert np.isin(pend, s).any() and np.isin(pend, d).any() and np.isin(queued, s).any()
    return s, d


def _rows_equal(out, src, dst, what, skip_obs=False):
    """obs / share_obs / rew / done / info rows of dst against src (info's diagnostics column aside), bit for bit."""
    import torch
    names = ("obs", "share_obs", "rew", "done", "info")
    si = torch.as_tensor(src, device=out[0].device)
    di = torch.as_tensor(dst, device=out[0].device)
    for nm, x in zip(names, out):
        if x is None or (skip_obs and nm in ("obs", "share_obs")):
            continue
        a, b = x[si], x[di]
        if nm == "info":
            a, b = a.clone(), b.clone()
            a[:, RSV] = 0
            b[:, RSV] = 0
        if not torch.equal(a, b):
            bad = (a != b).nonzero()
            raise AssertionError((what, nm, "pair", int(bad[0][0]), int(src[bad[0][0]]), int(dst[bad[0][0]]), bad[:4].tolist()))


def _bits(a):
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _state_equal(eng, src, dst, what):
    """Every state field's dst rows against its src rows, to the bit -- the four re-centring stamps aside (a request carries its
    slot in the request set, which two envs filing in the same step cannot share)."""
    pend = G.hdr_pend()
    for name in list(_CHECKPOINT) + list(_STATE_DTYPES) + ["ep_return"]:
        a = _bits(eng.get_state(name))
        x, y = a[src].copy(), a[dst].copy()
        if name == "header":
            x[:, pend] = 0
            y[:, pend] = 0
        if not np.array_equal(x, y):
            bad = np.nonzero((x != y).reshape(len(src), -1).any(axis=1))[0]
            raise AssertionError((what, name, [(int(src[k]), int(dst[k])) for k in bad[:4]]))


def _stagger(rig, g):
    """half the batch reset by mask after 10 steps: two groups 10 episode steps apart (the general kernel)"""
    import torch
    N = rig.N
    for _ in range(10):
        rig.eng.step(_acts(N, g))
    mask = np.arange(N) % 2 == 1
    rig.eng.reset(mask=mask)
    t = rig.eng.get_state("t_rel")
    assert len(np.unique(t)) == 2, np.unique(t)
    return torch


# (mapping, envs, mixed, staggered)
CASES = [
    ("pair", 4096, False, False),
    ("quad", 6144, False, False),
    ("wide", 8192, False, False),
    ("wide_gen", 8192, True, False),
    ("general", 2570, False, True),
]


@pytest.mark.parametrize("mapping,N,mixed,stagger", CASES, ids=[c[0] + "-" + str(c[1]) for c in CASES])
def test_a_clone_is_its_source_bit_for_bit(mapping, N, mixed, stagger):
    import torch
    rig = ProductionRig(N, mapping, mixed=mixed, episode_steps=EP, seed=900 + N, n_random=8, oracles=False)
    eng = rig.eng
    eng.reset()
    g = torch.Generator(device="cpu").manual_seed(N)
    rng = np.random.default_rng(N)
    if stagger:
        _stagger(rig, g)
    for _ in range(CLONE_AT):
        out = eng.step(_acts(N, g))
    while len(_pending_envs(eng)) < 2:      # (a step where re-centring requests of at least two envs are in flight)
        out = eng.step(_acts(N, g))
        assert eng.steps_to_episode_end() > 8
    kernel_before = eng.last_step_kernel()
    assert kernel_before == rig.geom.kernel, (kernel_before, rig.geom.kernel)
    src, dst = _pick_pairs(eng, rig.geom, rng)
    t_rel = eng.get_state("t_rel")
    obs, share = eng.clone_envs(src, dst)
    _rows_equal((obs, share, None, None, None), src, dst, "right after the clone")
    np.testing.assert_array_equal(eng.get_state("t_rel")[dst], t_rel[src])
    live = np.ones(len(src), bool)
    compared_state = False
    steps = 0
    while live.any():
        if not compared_state and eng.steps_to_episode_end() == 1:
            _state_equal(eng, src[live], dst[live], f"{mapping} {N} before the boundary")
            compared_state = True
        a = _acts(N, g)
        a[torch.as_tensor(dst)] = a[torch.as_tensor(src)]
        out = eng.step(a)
        if steps == 0 and not stagger:
            assert eng.last_step_kernel() == kernel_before, (eng.last_step_kernel(), kernel_before)
        done = out[3].cpu().numpy().astype(bool)
        ended = live & done[src]
        assert (done[src[live]] == done[dst[live]]).all()
        _rows_equal(out, src[live & ~ended], dst[live & ~ended], f"{mapping} {N} step {steps}")
        if ended.any():       # the done step: outputs and final_obs equal, obs is dst's own next episode
            _rows_equal(out, src[ended], dst[ended], f"{mapping} {N} done step {steps}", skip_obs=True)
            fo = eng.final_obs
            assert torch.equal(fo[torch.as_tensor(src[ended])], fo[torch.as_tensor(dst[ended])])
        live &= ~ended
        steps += 1
        assert steps <= EP + 1
    assert compared_state
    assert not bool((eng.info[:, L.INFO_IDX["fault"]] != 0).any())
    print(f"clone {mapping} {N}: {len(src)} pairs, kernel {kernel_before}, {steps} steps to the boundary")
    eng.close()


def _oracle_copy(o):
    """an independent oracle in the state of `o` (the C struct copied; the episode windows it points into are read-only)"""
    c = po.OracleEnv(o.p)
    C.memmove(C.byref(c.e), C.byref(o.e), C.sizeof(c.e))
    c._keep = o._keep
    return c


def test_divergent_branches_against_the_oracle_verify_mode():
    """Sampled envs cloned onto other sampled envs (their oracles copied likewise), then driven by DIFFERENT random actions than
    their sources: every sampled env against the fp64 oracle every step, through the auto-reset, where begin_all holds dst's draws
    to the NumPy restatement keyed on dst's own index.  debug_flags DEBUG_VERIFY: the verify kernel checks every env's reward state."""
    import torch
    N = 4096
    rig = ProductionRig(N, "pair", debug_flags=L.DEBUG_VERIFY, episode_steps=EP, seed=4242, n_random=160)
    eng = rig.eng
    obs, _ = eng.reset()
    rig.begin_all(obs)
    rig.single_steps(CLONE_AT, seed=5)
    s = np.array(rig.sample)
    t = 0
    while len(np.intersect1d(_pending_envs(eng), s)) < 2:     # (sampled envs with re-centring requests in flight: src's path changes)
        rig.single_steps(1, seed=100 + t)
        t += 1
        assert eng.steps_to_episode_end() > 8, "no sampled env with a request in flight"
    pend = np.intersect1d(_pending_envs(eng), s)
    rng = np.random.default_rng(7)
    rest = rng.permutation(np.setdiff1d(s, pend))
    k = len(s) // 3
    src = np.r_[pend[:max(1, len(pend) - 1)], rest[:k]][:k]      # (every pending env but one is a src, the last one a dst)
    dst = np.r_[pend[len(src[np.isin(src, pend)]):], rest[k:]][:k]
    assert np.isin(pend, src).any() and set(src).isdisjoint(dst) and len(set(dst)) == len(dst)
    eng.clone_envs(src, dst)
    for a, b in zip(src, dst):
        rig.orcs[int(b)] = _oracle_copy(rig.orcs[int(a)])
    resets = rig.resets
    rig.single_steps(EP - CLONE_AT + 6, seed=9)       # (independent actions per env: dst diverges from src)
    assert rig.resets == resets + 1
    print(f"divergent branches: {k} pairs, src with requests in flight {int(np.isin(src, pend).sum())}, dst "
          f"{int(np.isin(dst, pend).sum())}, worst {rig.worst}")
    rig.assert_ok()
    assert (eng.get_state("order_stat_sticky") == 0).all()
    eng.close()


def test_ring_mirror_at_49152_and_a_rollout_after_a_clone():
    """49 152 envs on the lane-per-env kernel read the evicted key from the ring's slot-major mirror: a contiguous dst block and a
    scattered set, bit for bit with their sources for 12 steps; then 16 384 envs, a clone, one rollout() of 12 steps."""
    import torch
    for N, mapping, use_rollout in ((49152, "wide", False), (16384, "wide", True)):
        rig = ProductionRig(N, mapping, episode_steps=EP, seed=31 + N, n_random=0, oracles=False, hist_cap=2048)
        eng = rig.eng
        eng.reset()
        g = torch.Generator(device="cpu").manual_seed(N)
        for _ in range(CLONE_AT):
            eng.step(_acts(N, g))
        kernel = eng.last_step_kernel()
        rng = np.random.default_rng(N)
        block_src, block_dst = np.arange(1000, 1640), np.arange(N - 2000, N - 1360)
        others = np.setdiff1d(np.arange(N), np.r_[block_src, block_dst])
        sc = rng.choice(others, 128, replace=False)
        src, dst = np.r_[block_src, sc[:64]], np.r_[block_dst, sc[64:]]
        eng.clone_envs(src, dst)
        if use_rollout:
            acts = torch.randint(0, 3, (12, N, 3), dtype=torch.int32, generator=g).cuda()
            acts[:, torch.as_tensor(dst)] = acts[:, torch.as_tensor(src)]
            out = eng.rollout(acts)
            assert eng.last_step_kernel() == kernel
            for t in range(12):
                _rows_equal([x[t] for x in out], src, dst, f"rollout {N} step {t}")
        else:
            for t in range(12):
                a = _acts(N, g)
                a[torch.as_tensor(dst)] = a[torch.as_tensor(src)]
                out = eng.step(a)
                assert eng.last_step_kernel() == kernel
                _rows_equal(out, src, dst, f"{N} step {t}")
        _state_equal(eng, src, dst, f"{N} after 12 steps")
        print(f"mirror / rollout {N}: {len(src)} pairs, kernel {kernel}")
        eng.close()


def _actor(seed):
    r = np.random.default_rng(seed)
    p = {k: r.normal(0, 0.4, shape).astype(np.float32) for k, shape in
         (("w1", (64, 26)), ("b1", (64,)), ("w2", (64, 64)), ("b2", (64,)), ("w3", (3, 64)), ("b3", (3,)))}
    for k, n in (("ln0", 26), ("ln1", 64), ("ln2", 64)):
        p[k + "_gamma"] = (1 + r.normal(0, 0.1, n)).astype(np.float32)
        p[k + "_beta"] = r.normal(0, 0.1, n).astype(np.float32)
    return p


def test_rollout_actor_right_after_a_clone():
    """The closed loop chooses its first actions from the library's copy of the latest observations: after a clone the dst rows of
    the actions and the logits (mode, not draws: draws are keyed on the env's index) equal the src rows, as do all outputs."""
    import torch
    N = 4096
    rig = ProductionRig(N, "pair", episode_steps=EP, seed=77, n_random=0, oracles=False)
    eng = rig.eng
    for a in range(3):
        eng.set_actor(a, _actor(10 + a))
    eng.reset()
    g = torch.Generator(device="cpu").manual_seed(3)
    for _ in range(CLONE_AT):
        eng.step(_acts(N, g))
    rng = np.random.default_rng(3)
    perm = rng.permutation(N)
    src, dst = perm[:200], perm[200:400]
    eng.clone_envs(src, dst)
    out = eng.rollout_actor(12, sample=False, want_logits=True)
    acts, logits = out[5], out[6]
    assert torch.equal(acts[:, torch.as_tensor(src)], acts[:, torch.as_tensor(dst)])
    assert torch.equal(logits[:, torch.as_tensor(src)], logits[:, torch.as_tensor(dst)])
    assert len(torch.unique(acts[:, torch.as_tensor(src)])) == 3
    for t in range(12):
        _rows_equal([x[t] for x in out[:5]], src, dst, f"closed loop step {t}")
    eng.close()


def _small(n=64, steps=16, reset=True):
    tb = traces.synthetic_tables("ny", 0)
    p = dc_config.size_datacenter("dc_config.json", 1, 30.0)
    e = SdcEngine(n, episode_steps=steps, auto_reset=True, seed=5)
    e.set_tables(0, tb["W"], tb["C"], tb["T"], tb["WB"])
    e.set_dc_params(0, p)
    e.assign(0, 0, 174, 188)
    if reset:
        e.reset()
    return e


def test_refusals_change_nothing():
    import torch
    e = _small()
    g = torch.Generator(device="cpu").manual_seed(1)
    for _ in range(5):
        e.step(_acts(64, g))
    before = {k: e.get_state(k) for k in _CHECKPOINT}
    obs0 = e.obs.clone()
    left = e.steps_to_episode_end()
    bad = [
        ([], [], "n must be positive"),
        ([1], [64], "outside"),
        ([-1], [3], "outside"),
        ([1, 2], [5, 5], "twice"),
        ([1, 5], [5, 6], "both a src and a dst"),
        ([1, 2], [3], "sources for"),
    ]
    for s, d, msg in bad:
        with pytest.raises(ValueError, match=msg):
            e.clone_envs(s, d)
    # the library's own checks, without the binding's
    ip = C.POINTER(C.c_int32)
    for s, d, msg in (([0], [64], b"outside"), ([0], [-2], b"outside"), ([3, 4], [7, 7], b"twice"), ([3, 7], [7, 8], b"both")):
        sa, da = np.array(s, np.int32), np.array(d, np.int32)
        rc = e.lib.sdc_clone_envs(e._h, sa.ctypes.data_as(ip), da.ctypes.data_as(ip), len(s), None, None, None)
        assert rc == -2 and msg in e.lib.sdc_last_error(), (s, d, rc, e.lib.sdc_last_error())
    assert e.lib.sdc_clone_envs(e._h, None, None, 1, None, None, None) == -2
    assert e.lib.sdc_clone_envs(None, None, None, 1, None, None, None) == -2
    assert b"null handle" in e.lib.sdc_last_error()
    for k in _CHECKPOINT:
        np.testing.assert_array_equal(_bits(e.get_state(k)), _bits(before[k]), err_msg=k)
    assert torch.equal(e.obs, obs0) and e.steps_to_episode_end() == left
    fresh = _small(reset=False)
    with pytest.raises(ValueError, match="sdc_reset"):
        fresh.clone_envs([0], [1])
    # and a clone that is allowed: a scalar src broadcast over several dst
    e.clone_envs(3, [10, 11, 12])
    for k in ("record", "hist", "qtab"):
        v = _bits(e.get_state(k))
        assert (v[[10, 11, 12]] == v[3]).all(), k
    assert torch.equal(e.obs[[10, 11, 12]], e.obs[[3, 3, 3]])
    fresh.close()
    e.close()


def test_vec_env_clone_returns_reset_layout():
    """SustainDCVecEnv.clone_envs: (obs, share_obs, available_actions) in reset()'s layout, for an agent subset with the
    concatenated shared observation and for all three agents with the 29-float one."""
    import torch
    ENV_ARGS = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True}
    for agents, concat in ((["agent_dc", "agent_bat"], False), (["agent_ls", "agent_dc", "agent_bat"], True)):
        args = dict(ENV_ARGS, agents=agents, nonoverlapping_shared_obs_space=concat)
        env = SustainDCVecEnv(args, n_envs=16, seed=3, months=[6] * 16)
        o0, s0, a0 = env.reset()
        env.step(np.ones((16, len(agents)), np.int32))
        o, s, a = env.clone_envs(2, [7, 9])
        assert o.shape == o0.shape and s.shape == s0.shape and a.shape == a0.shape, (o.shape, s.shape)
        np.testing.assert_array_equal(o[[7, 9]], o[[2, 2]])
        np.testing.assert_array_equal(s[[7, 9]], s[[2, 2]])
        r = env.step(np.ones((16, len(agents)), np.int32))
        np.testing.assert_array_equal(r[0][[7, 9]], r[0][[2, 2]])
        np.testing.assert_array_equal(r[2][[7, 9]], r[2][[2, 2]])
        with pytest.raises(ValueError):
            env.clone_envs([1], [1])
        env.close()


def _info_dict(row):
    return {k: row[k] for k in row.keys()}


def test_vec_env_clone_across_configs_carries_the_info_constants():
    """A batch of two data-centre configs: cloning an env of one onto envs of the other gives dst src's config on the device AND
    in the host's per-env info constants (power bounds, pump powers, battery capacity): every entry of infos[dst] equals infos[src]
    on the next steps -- the diagnostics column aside -- while the infos of the step before the clone keep dst's old constants."""
    args = [{"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True,
             "dc_config_file": ("dc_config.json", "dc_config_r16.json")[i % 2]} for i in range(16)]
    env = SustainDCVecEnv(args, n_envs=16, seed=3, months=[6] * 16)
    env.reset()
    before = env.step(np.ones((16, 3), np.int32))[4]
    old = _info_dict(before[3][0])
    assert old["dc_power_ub_kW"] != _info_dict(before[0][0])["dc_power_ub_kW"]     # (the two configs differ)
    env.clone_envs(0, [3, 5])
    assert env._cfg_id[3] == env._cfg_id[5] == env._cfg_id[0]
    np.testing.assert_array_equal(env.engine.get_state("cfg_id")[[3, 5]], env.engine.get_state("cfg_id")[[0, 0]])
    assert _info_dict(before[3][0])["dc_power_ub_kW"] == old["dc_power_ub_kW"]      # (an earlier step's infos are unchanged)
    rng = np.random.default_rng(1)
    for t in range(3):
        a = rng.integers(0, 3, (16, 3)).astype(np.int32)
        a[[3, 5]] = a[0]
        infos = env.step(a)[4]
        for e in (3, 5):
            for ag in range(3):
                x, y = _info_dict(infos[0][ag]), _info_dict(infos[e][ag])
                assert x.keys() == y.keys()
                for k in x:
                    if k != "reserved":
                        assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), (t, e, ag, k, x[k], y[k])
    env.close()


def test_back_to_back_clones_without_a_wait_in_between():
    """Three clones queued one after the other (the staging buffers are used in turn), then a step: each dst holds its own src."""
    import torch
    e = _small(n=128)
    g = torch.Generator(device="cpu").manual_seed(2)
    for _ in range(3):
        e.step(_acts(128, g))
    want = e.get_state("record")
    for s, d in ((3, [40, 41]), (4, [50]), (5, [60, 61, 62])):
        e.clone_envs(s, d)
    got = e.get_state("record")
    for s, d in ((3, [40, 41]), (4, [50]), (5, [60, 61, 62])):
        assert (got[d] == want[s]).all(), (s, d)
    e.step(_acts(128, g))
    e.close()
