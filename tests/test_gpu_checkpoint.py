"""Checkpoint restore (SdcEngine.state_dict / load_state_dict over sdc_get_state / sdc_set_state) under the oracles, on every
step mapping.  A restore is not a plain copy: sdc_set_state drops and restores the order-statistic trackers, rebuilds the queue
table's time-major mirror (from 7 680 envs) and the ring's slot-major mirror (from 49 152), rebuilds the per-env config scalars
from a `record` of several configs, moves the launch counter past every in-flight re-centring stamp and invalidates the feature
rows -- so a restored engine ("B") runs the general kernels until its next episode boundary, then the specialised ones again.

Every case holds B's sampled envs to the fp64 oracle on every step, EVERY env of B bit for bit to the engine the checkpoint came
from ("A", stepped alongside), continues past B's first auto-reset (whose draws begin_all holds to the NumPy restatement of the
device's Philox scheme: that is what catches a lost seed, env_index_base or episode counter) and at the end compares A's and B's
whole state array by array.  Plus: the checkpoint's "meta" (state layout, configuration, seed) and the refusals it allows."""
import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import dc_config, traces
from dc_rl_amd.engine import SdcEngine
from tests import gpu_helpers as G
from tests import parity_util as P
from tests.production_rig import ProductionRig

pytestmark = pytest.mark.gpu

TOL = 1e-5
EP = 64          # episode_steps of the restore cases: short episodes, so that B's boundary comes soon
AFTER = 24       # single steps on the specialised kernel after B's first boundary


def _acts(N, g):
    import torch
    return torch.randint(0, 3, (N, 3), dtype=torch.int32, generator=g).cuda()


def _pending(sd):
    """envs with a deferred re-centring request in flight in a checkpoint's headers"""
    return int((sd["header"][:, G.hdr_pend()] != 0).any(axis=1).sum())


def _bits(a):
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a.view(np.uint32)


def _window_fields():
    """header dwords of the four rank windows {Q1, Q3, upper bound, lower bound} (qwin's lane order): (r0, hi) of each, their
    first and last keys"""
    h = G.hdr_offsets()
    tracks = [h["H_Q1"], h["H_Q3"], h["H_BU"], h["H_BL"]]
    first = [h["H_WFIRST"] + w for w in range(4)]
    last = [h["H_WLAST"] + w for w in range(4)]
    return tracks, first, last


def _check_windows(hdr, qwin, tracks, first, last, who):
    """A header's rank windows describe its own qwin (where the reward state is valid): the first / last key dwords are lanes 0
    and hi - 1 of the window (what sdc_reward_verify_kernel holds them to)."""
    valid = hdr[:, G.hdr_offsets()["H_VALID"]] == 1
    for w, t in enumerate(tracks):
        hi = hdr[:, t + 1].astype(np.int64)
        ok = valid & (hi > 0)
        assert (hi[ok] <= qwin.shape[1]).all(), (who, w)
        e = np.nonzero(ok)[0]
        assert (hdr[e, first[w]] == qwin[e, 0, w]).all(), (who, "first key", w)
        assert (hdr[e, last[w]] == qwin[e, hi[e] - 1, w]).all(), (who, "last key", w)


def _ring_keys(row, complemented):
    """one env's ring (fp32 offsets, NaN = empty) -> its device keys (sdc_trackers.hpp f32_key), ascending"""
    b = row[~np.isnan(row)].view(np.uint32)
    k = b ^ ((b.view(np.int32) >> 31).view(np.uint32) | np.uint32(0x80000000))
    return np.sort(~k if complemented else k)


def _check_ranks(hist, hdr, qwin, e, w, t, who):
    """every key of env e's window w against its rank in the ring: lane i's key v satisfies #{x < v} <= r0 + i < #{x <= v}
    (sdc_verify.hip; the lower clip bound's window lives on complemented keys)"""
    r0, n = int(hdr[e, t]), int(hdr[e, t + 1])
    ks = _ring_keys(hist[e], w == 3)
    v = qwin[e, :n, w]
    r = r0 + np.arange(n)
    assert ((np.searchsorted(ks, v, "left") <= r) & (r < np.searchsorted(ks, v, "right"))).all(), (who, "window ranks", int(e), w)


def assert_same_state(a, b, what):
    """A's and B's state_dict() array by array, to the bit -- except where the two may legitimately differ:
      * H_PEND, the launch-counter stamps of in-flight re-centring requests (a restore moves B's launch counter on);
      * the PLACEMENT of the four rank windows (r0 / hi, first / last key, the qwin lanes).  A window caches 64 consecutive order
        statistics of the ring around a wanted rank; it is re-centred by a deferred request, and B drops the requests in flight
        at the restore (stale stamps) and re-requests them from other steps, so its windows may sit a few ranks off A's.  What
        they cache must agree: on the ranks both windows of an env hold, the keys are the same bits (the rings themselves are
        compared in full), and each engine's first / last key dwords are those of its own window.
      * the last bits of the header's fp64 running sums: the totals A1 / A2 and the clip bounds' tail sums, and the episode
        returns that accumulate the fp64 rewards computed from them.  A step whose clip bound has left its window takes the sums
        fresh from the ring (sdc_pairstep.hpp ring_sums, "why" 5-7; likewise a rebuild) instead of carrying them on incrementally --
        the same quantities, rounded differently -- and with its windows placed differently B takes that path at other steps than
        A.  All six sums and the returns are held to the bar the verify kernel applies to A1 alone (1e-9 relative with the history
        length as slack, sdc_verify.hip) -- a bound chosen here, not one the kernels promise for the tail sums.  Every fp32 output,
        the returns in the info rows included, is still held to the bit by the cases: with these seeds no such last-bit difference
        crosses an fp32 rounding boundary.  Other seeds may make one do so (a reward one fp32 ulp apart) without a defect behind it.
    -> the number of (env, window) pairs whose placement differs."""
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["meta"] == sb["meta"], (what, sa["meta"], sb["meta"])
    tracks, first, last = _window_fields()
    h = G.hdr_offsets()
    sums = [h["H_QS2_LO"], h["H_QS1"], h["H_QS1"] + 2, h["H_QS2_HI"], h["H_A1"], h["H_A2"]]
    rets = [h["H_RET"] + 2 * j for j in range(3)]
    f64 = lambda hd, k: np.ascontiguousarray(hd[:, k:k + 2]).view(np.float64)[:, 0]
    for cols, slack in ((sums, float(a.config["hist_cap"])), (rets, 1.0)):
        for k in cols:
            x, y = f64(sa["header"], k), f64(sb["header"], k)
            assert (np.abs(x - y) <= 1e-9 * (np.abs(x) + slack)).all(), (what, "header f64 at dword", k)
    masked = (G.hdr_pend() + [t + j for t in tracks for j in (0, 1)] + first + last +
              [k + j for k in sums + rets for j in (0, 1)])
    diffs = {}
    for k in sa:
        if k in ("meta", "qwin"):
            continue
        x, y = _bits(sa[k]), _bits(sb[k])
        assert x.shape == y.shape, (what, k)
        if k == "header":
            x, y = x.copy(), y.copy()
            x[:, masked] = 0
            y[:, masked] = 0
        if not np.array_equal(x, y):
            bad = np.nonzero(x != y)
            diffs[k] = (len(bad[0]), [tuple(int(i) for i in j) for j in zip(*bad)][:4])
    assert not diffs, (what, diffs)
    ha, hb, qa, qb = sa["header"], sb["header"], sa["qwin"], sb["qwin"]
    _check_windows(ha, qa, tracks, first, last, "A")
    _check_windows(hb, qb, tracks, first, last, "B")
    moved = 0
    for w, t in enumerate(tracks):
        for e in np.nonzero((ha[:, [t, t + 1]] != hb[:, [t, t + 1]]).any(axis=1) | (qa[:, :, w] != qb[:, :, w]).any(axis=1))[0]:
            ra, na, rb, nb = int(ha[e, t]), int(ha[e, t + 1]), int(hb[e, t]), int(hb[e, t + 1])
            lo, hi = max(ra, rb), min(ra + na, rb + nb)
            if hi > lo:
                assert np.array_equal(qa[e, lo - ra:hi - ra, w], qb[e, lo - rb:hi - rb, w]), (what, "window keys", int(e), w)
            if moved < 64:       # (and the first few against the ring itself)
                _check_ranks(sa["hist"], ha, qa, e, w, t, (what, "A"))
                _check_ranks(sb["hist"], hb, qb, e, w, t, (what, "B"))
            moved += 1
    return moved


def _run_past_boundary(rig, g, after=AFTER):
    """Single steps of the restored rig until AFTER steps past B's first episode boundary."""
    n = 0
    while rig.restored == "general":
        rig.step(_acts(rig.N, g))
        n += 1
        assert n <= rig.steps + 1
    for _ in range(after):
        rig.step(_acts(rig.N, g))
    assert rig.restore_kernels["specialised"] == {rig.geom.kernel}, rig.restore_kernels


def _t_rel(rig):
    return rig.steps - rig.eng.steps_to_episode_end()


def _steps_to(rig, g, t_rel):
    while _t_rel(rig) != t_rel:
        rig.step(_acts(rig.N, g))


# (mapping, envs, mixed, snapshot points): mid = mid-episode with requests in flight, last = t_rel episode_steps - 1,
# first = right after an auto-reset, before the new episode's first step (t_rel 0)
MAPPINGS = [
    ("pair", 4096, False, ("mid", "last", "first")),
    ("quad", 6144, False, ("mid",)),
    ("wide", 8192, False, ("mid", "last", "first")),
    ("wide", 49152, False, ("mid",)),            # the ring's slot-major mirror (SdcDev::hist_t)
    ("wide_gen", 16384, True, ("mid",)),         # configs[3]: nine configs, the lane-per-env kernel's general form
]


@pytest.mark.parametrize("mapping,N,mixed,points", MAPPINGS, ids=[f"{m[0]}-{m[1]}" for m in MAPPINGS])
def test_restore_into_a_fresh_engine_vs_oracle_and_twin(mapping, N, mixed, points):
    """Full rings, debug_flags 0, auto-reset: at each snapshot point restore into a fresh engine with the rig's arguments, step it
    with the sampled oracles and the old engine alongside past its first boundary and AFTER steps on, then compare the states."""
    import torch
    rig = ProductionRig(N, mapping, debug_flags=0, mixed=mixed, episode_steps=EP, seed=4000 + N, n_random=40)
    obs, _ = rig.eng.reset()
    rig.begin_all(obs)
    g = torch.Generator(device="cpu").manual_seed(N)
    pend = {}
    for pt in points:
        _steps_to(rig, g, {"mid": 30, "last": EP - 1, "first": 0}[pt])
        if rig.twin is not None:       # (the next restore checkpoints B: the old twin has done its work)
            rig.twin.close()
            rig.twin = None
        sd = rig.restore()
        pend[pt] = _pending(sd)
        if pt == "mid":
            assert pend[pt] > 0, pend
        _run_past_boundary(rig, g)
        moved = assert_same_state(rig.twin, rig.eng, f"{mapping} {N} after the {pt} snapshot")
        print(f"{mapping} {N} {pt}: twin ran {sorted(rig.twin_kernels)}, B ran {rig.restore_kernels}, "
              f"rank windows placed differently {moved}")
        rig.restore_kernels = {"general": set(), "specialised": set()}
        rig.twin_kernels = set()
    print(f"{mapping} {N}: worst {rig.worst}, envs with requests in flight at the snapshots {pend}, resets {rig.resets}")
    assert rig.resets >= len(points)
    rig.assert_ok()
    assert (rig.eng.get_state("order_stat_sticky") == 0).all()
    rig.twin.close()
    rig.eng.close()


ROLLOUTS = [(8192, "sdc_rollout_quad_kernel"), (16384, "sdc_dynamics_wide_kernel")]


@pytest.mark.parametrize("N,a_kernel", ROLLOUTS, ids=[str(r[0]) for r in ROLLOUTS])
def test_rollout_after_a_restore_vs_oracle_and_twin(N, a_kernel):
    """rollout(K) on A and on the restored B up to the boundary and past it: B has no feature rows, so it runs the multi-step
    sdc_rollout_kernel (inline re-centring, full rings) until its boundary, then what A runs -- one sdc_rollout_quad_kernel launch
    at 8 192 envs, K lane-per-env launches at 16 384."""
    import torch
    rig = ProductionRig(N, "wide", debug_flags=0, episode_steps=EP, seed=5000 + N, n_random=40)
    obs, _ = rig.eng.reset()
    rig.begin_all(obs)
    g = torch.Generator(device="cpu").manual_seed(N + 1)
    _steps_to(rig, g, 30)
    sd = rig.restore()
    a, b = rig.twin, rig.eng
    b_kernels = []
    past = 0
    while past < AFTER:
        k = min(24, b.steps_to_episode_end())
        acts = torch.randint(0, 3, (k, N, 3), dtype=torch.int32, generator=g).cuda()
        out_a = a.rollout(acts)
        assert a.last_step_kernel() == a_kernel
        out_b = b.rollout(acts)
        b_kernels.append(b.last_step_kernel())
        rig.check_rollout(acts, out_b)
        rig.twin_equal(out_a, out_b, "rollout", final_obs=bool(out_b[3][-1].any()))
        if rig.restored == "specialised":
            assert b_kernels[-1] == a_kernel, b_kernels
            past += k
        else:
            assert b_kernels[-1] == "sdc_rollout_kernel", b_kernels
        if b.steps_to_episode_end() == rig.steps:
            rig.resets += 1
            rig.restored = "specialised"
            rig.begin_all(out_b[0][-1])
    print(f"rollout after a restore, {N} envs: A ran {a_kernel}, B ran {b_kernels}, worst {rig.worst}, "
          f"envs with requests in flight at the snapshot {_pending(sd)}")
    rig.assert_ok()
    print("rank windows placed differently:", assert_same_state(a, b, f"rollout {N}"))
    a.close()
    b.close()


def test_policy_rollout_after_a_restore_16384_mixed():
    """rollout_policy with the rule-based policies (do-nothing ls, trim-and-respond, RBC battery) and tou_reward for the dc agent on
    the configs[3] mix at 16 384 envs: A runs K launches of the lane-per-env kernel's general form, the restored B the multi-step
    sdc_rollout_kernel until its boundary; the actions the policies chose and every output of every env the same bits."""
    import torch
    N = 16384
    rig = ProductionRig(N, "wide_gen", debug_flags=0, mixed=True, episode_steps=EP, seed=5161, n_random=40,
                        reward_method=(0, 3, 0), policy=(1, 3, 2), trim_and_respond_limit=28.5)
    eng = rig.eng
    obs, _ = eng.reset()
    rig.begin_all(obs)
    out = eng.rollout_policy(30)
    rig.check_rollout(out[5], out)
    sd = rig.restore()
    a, b = rig.twin, rig.eng
    b_kernels = []
    past = 0
    while past < AFTER:
        k = min(24, b.steps_to_episode_end())
        out_a = a.rollout_policy(k)
        assert a.last_step_kernel() == "sdc_dynamics_wide_gen_kernel"
        out_b = b.rollout_policy(k)
        b_kernels.append(b.last_step_kernel())
        assert torch.equal(out_a[5], out_b[5]), "the policies' actions"
        rig.check_rollout(out_b[5], out_b)
        rig.twin_equal(out_a, out_b, "policy rollout", final_obs=bool(out_b[3][-1].any()))
        if rig.restored == "specialised":
            assert b_kernels[-1] == "sdc_dynamics_wide_gen_kernel", b_kernels
            past += k
        else:
            assert b_kernels[-1] == "sdc_rollout_kernel", b_kernels
        if b.steps_to_episode_end() == rig.steps:
            rig.resets += 1
            rig.restored = "specialised"
            rig.begin_all(out_b[0][-1])
    print(f"policy rollout after a restore, {N} envs: B ran {b_kernels}, worst {rig.worst}, "
          f"envs with requests in flight at the snapshot {_pending(sd)}")
    assert len(np.unique(out_b[5][:, :, 1].cpu().numpy())) >= 2
    rig.assert_ok()
    print("rank windows placed differently:", assert_same_state(a, b, "policy rollout"))
    a.close()
    b.close()


REWINDS = [("wide", 8192, False), ("wide_gen", 16384, True)]


@pytest.mark.parametrize("mapping,N,mixed", REWINDS, ids=[f"{r[0]}-{r[1]}" for r in REWINDS])
def test_rewind_on_the_same_engine_across_the_boundary(mapping, N, mixed):
    """state_dict(), 72 single steps (the oracles check them; the episode boundary is among them), load_state_dict() on the SAME
    engine and the same 72 steps again: every output of every env the same bits, verify mode on (debug_flags DEBUG_VERIFY: every step's
    reward state checked against an exact pass over the ring), requests in flight at the checkpoint."""
    import torch
    rig = ProductionRig(N, mapping, debug_flags=L.DEBUG_VERIFY, mixed=mixed, episode_steps=EP, seed=6000 + N, n_random=24)
    eng = rig.eng
    obs, _ = eng.reset()
    rig.begin_all(obs)
    g = torch.Generator(device="cpu").manual_seed(N + 2)
    _steps_to(rig, g, 30)
    sd = eng.state_dict()
    pend = _pending(sd)
    acts = [_acts(N, g) for _ in range(72)]
    first = []
    for t in range(72):
        out = rig.step(acts[t])
        first.append([x.clone() for x in out] + [eng.final_obs.clone()])
    assert rig.resets >= 1
    eng.load_state_dict(sd)
    kernels = []
    for t in range(72):
        out = eng.step(acts[t])
        kernels.append(eng.last_step_kernel())
        again = [x.clone() for x in out] + [eng.final_obs.clone()]
        for u, v, nm in zip(first[t], again, ("obs", "share_obs", "rew", "done", "info", "final_obs")):
            if nm == "info":
                u, v = u.clone(), v.clone()
                u[:, L.INFO_IDX["reserved"]] = 0
                v[:, L.INFO_IDX["reserved"]] = 0
            if nm == "final_obs" and not bool(first[t][3].any()):
                continue        # (written at an episode end only)
            assert torch.equal(u, v), (t, nm)
    boundary = EP - 30
    assert kernels[:boundary] == ["sdc_dynamics_kernel"] * boundary, kernels
    assert set(kernels[boundary:]) == {rig.geom.kernel}, kernels
    print(f"rewind {mapping} {N}: worst {rig.worst}, envs with requests in flight {pend}, kernels after the rewind "
          f"{kernels[0]} x {boundary}, {kernels[-1]} x {72 - boundary}")
    assert pend > 0
    assert (eng.info[:, L.INFO_IDX["fault"]] == 0).all()
    assert (eng.get_state("order_stat_sticky") == 0).all()
    rig.assert_ok()
    eng.close()


ONE_STEP = [("pair", 4096), ("wide", 8192)]


@pytest.mark.parametrize("mapping,N", ONE_STEP, ids=[f"{m[0]}-{m[1]}" for m in ONE_STEP])
def test_one_step_rewind_takes_over_no_stale_window(mapping, N):
    """state_dict(), ONE step, load_state_dict() on the same engine, the same step again -- the one rewind after which requests
    stamped in the step before the checkpoint would look exactly "two steps old" to the replayed step, whose launch counter is
    one on from the checkpoint's: without sdc_set_state moving the counter on, the replay would take over the window swept for
    the first pass, which already holds the replayed step's own insertion, and replay that insertion a second time.  Verify mode
    (debug_flags DEBUG_VERIFY) checks every window against the ring after every step; the replay must equal the first pass to the bit.
    Four rounds, one per episode, late in the episode where requests are many; the first pass runs the kernel of the mapping
    (the episode boundary between the rounds brings the feature rows back), the replay the general kernel."""
    import torch
    rig = ProductionRig(N, mapping, debug_flags=L.DEBUG_VERIFY, episode_steps=EP, seed=8000 + N, n_random=24)
    eng = rig.eng
    obs, _ = eng.reset()
    rig.begin_all(obs)
    g = torch.Generator(device="cpu").manual_seed(N + 4)
    rsv = L.INFO_IDX["reserved"]
    pend = []
    for t_snap in (62, 55, 48, 40):
        _steps_to(rig, g, t_snap)
        sd = eng.state_dict()
        pend.append(_pending(sd))
        a1 = _acts(N, g)
        first = [x.clone() for x in rig.step(a1)] + [eng.final_obs.clone()]
        assert eng.last_step_kernel() == rig.geom.kernel
        eng.load_state_dict(sd)
        again = [x.clone() for x in eng.step(a1)] + [eng.final_obs.clone()]
        assert eng.last_step_kernel() == "sdc_dynamics_kernel"
        for u, v, nm in zip(first, again, ("obs", "share_obs", "rew", "done", "info", "final_obs")):
            if nm == "info":
                u[:, rsv] = 0
                v[:, rsv] = 0
            if nm == "final_obs" and not bool(first[3].any()):
                continue
            assert torch.equal(u, v), (t_snap, nm)
        assert (eng.info[:, L.INFO_IDX["fault"]] == 0).all(), t_snap
        # (the oracles took the first pass, which the replay has just repeated: they go on from here)
        rig.single_steps(4, seed=t_snap)
    rig.single_steps(EP - 40 + 2, seed=1)       # (past the last round's boundary: the specialised kernel again)
    print(f"one-step rewind {mapping} {N}: worst {rig.worst}, envs with requests in flight at the checkpoints {pend}")
    assert sum(pend) > 0
    assert (eng.get_state("order_stat_sticky") == 0).all()
    rig.assert_ok()
    eng.close()


@pytest.mark.parametrize("mapping,N", [("pair", 4096), ("wide_gen", 8192)])
def test_multi_config_record_restores_the_assignment(mapping, N):
    """B built with EVERY env assigned to config 0, then a checkpoint of the configs[3] mix loaded: B follows the record -- its
    cfg_id, its per-env copies of the configs' scalars (what the two-env kernel of several configs reads: rebuild_prm_env) and,
    after the boundary, the lane-per-env kernel's per-config tables -- against the oracles and A."""
    import torch
    rig = ProductionRig(N, mapping, debug_flags=0, mixed=True, episode_steps=EP, seed=7000 + N, n_random=40)
    obs, _ = rig.eng.reset()
    rig.begin_all(obs)
    g = torch.Generator(device="cpu").manual_seed(N + 3)
    _steps_to(rig, g, 30)
    rig.restore(cfg_id=np.zeros(N, np.int32))
    np.testing.assert_array_equal(rig.eng.get_state("cfg_id"), rig.cfg_id)
    _run_past_boundary(rig, g)
    print(f"multi-config record {mapping} {N}: worst {rig.worst}, twin ran {sorted(rig.twin_kernels)}, B ran {rig.restore_kernels}")
    rig.assert_ok()
    print("rank windows placed differently:", assert_same_state(rig.twin, rig.eng, f"multi-config {N}"))
    rig.twin.close()
    rig.eng.close()


def test_staggered_envs_and_partial_rings_restore_vs_oracle():
    """2 570 envs (an odd grid of two-env workgroups with the sweep workgroups inside it), EVERY env against the oracle, rings
    filling from empty: half the envs reset by mask mid-episode, the checkpoint taken while the two halves sit at different
    episode steps (rel_hint -1), restored into a fresh engine that then steps past each half's own boundary, bit for bit with A."""
    import torch
    N, steps, seed = 2570, EP, 2570
    rig = P.ParityRig(N, episode_steps=steps, seed=seed)
    worst = dict(obs=0.0, rew=0.0, info=0.0)
    arng = np.random.default_rng(seed + 1)

    def reset_check(eobs, oobs):
        for i, o in oobs.items():
            worst["obs"] = max(worst["obs"], float(G.rel_err(eobs[i], o).max()))

    cols = [P.po.INFO_IDX[k] for k in P.INFO_CMP]

    def compare_step(acts):
        """P.compare_step for every env at once (one vectorised comparison instead of one per env and column)"""
        eo, es, er, ed, ei = rig.step(acts)
        np.testing.assert_array_equal(es, G.share_from_raw(eo))
        res = [rig.oracles[i].step(acts[i]) for i in range(N)]
        oo, orew = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
        odone, oinfo = np.array([r[2] for r in res]), np.stack([r[3] for r in res])
        np.testing.assert_array_equal(ed.astype(int), odone)
        worst["obs"] = max(worst["obs"], float(G.rel_err(eo, oo).max()))
        worst["rew"] = max(worst["rew"], float(G.rel_err(er, orew).max()))
        worst["info"] = max(worst["info"], float(G.rel_err(ei[:, cols], oinfo[:, cols]).max()))
        assert (ei[:, L.INFO_IDX["fault"]] == 0).all() and (oinfo[:, P.po.INFO_IDX["fault"]] == 0).all()
        return ed

    reset_check(*rig.reset_all())
    t_rel = np.zeros(N, int)
    half = np.arange(N) % 2 == 1
    for t in range(20):
        compare_step(arng.integers(0, 3, (N, 3)).astype(np.int32))
        t_rel += 1
    reset_check(*rig.reset_some(half))
    t_rel[half] = 0
    for t in range(10):
        compare_step(arng.integers(0, 3, (N, 3)).astype(np.int32))
        t_rel += 1
    np.testing.assert_array_equal(rig.eng.get_state("t_rel"), t_rel)
    assert len(np.unique(t_rel)) == 2
    a = rig.eng
    sd = a.state_dict()
    hl = a.get_state("hist_len").astype(np.int64)
    assert 0 < hl.max() < 10000, hl.max()
    b = SdcEngine(N, episode_steps=steps, auto_reset=False, seed=seed, debug_flags=L.DEBUG_VERIFY)
    tb = rig.tables[0]
    b.set_tables(0, tb["W"], tb["C"], tb["T"], tb["WB"])
    b.set_dc_params(0, rig.params[0])
    b.assign(rig.loc_id, rig.cfg_id, rig.day_lo, rig.day_hi)
    b.reset()
    b.load_state_dict(sd)
    assert b.steps_to_episode_end() == steps - t_rel.max()
    rig.eng = b
    rsv = L.INFO_IDX["reserved"]
    boundaries = 0
    while boundaries < 2 or t_rel.min() < 8:
        acts = arng.integers(0, 3, (N, 3)).astype(np.int32)
        ed = compare_step(acts)
        out_a = a.step(torch.from_numpy(acts).to(a.device))
        for nm, u, v in zip(("obs", "share_obs", "rew", "done", "info"), out_a, (b.obs, b.share_obs, b.rew, b.done, b.info)):
            if nm == "info":
                u, v = u.clone(), v.clone()
                u[:, rsv] = 0
                v[:, rsv] = 0
            assert torch.equal(u, v), nm
        assert b.last_step_kernel() == "sdc_dynamics_kernel"
        t_rel += 1
        np.testing.assert_array_equal(ed.astype(bool), t_rel >= steps)
        if ed.any():
            assert not ed.all()              # (each half reaches its own boundary)
            mask = t_rel >= steps
            reset_check(*rig.reset_some(mask, also=(a,)))
            t_rel[mask] = 0
            boundaries += 1
    print("staggered restore, 2570 envs:", worst, "episode ends after the restore:", boundaries)
    assert worst["obs"] <= TOL and worst["rew"] <= TOL and worst["info"] <= 2e-6
    print("rank windows placed differently:", assert_same_state(a, b, "staggered"))
    assert (b.get_state("order_stat_sticky") == 0).all()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- the checkpoint's "meta"
def _small(n=64, steps=16, seed=11, **kw):
    tb = traces.synthetic_tables("ny", 0)
    p = dc_config.size_datacenter("dc_config.json", 1, 30.0)
    e = SdcEngine(n, episode_steps=steps, auto_reset=True, seed=seed, **kw)
    for li in range(kw.get("n_locations", 1)):
        e.set_tables(li, tb["W"], tb["C"], tb["T"], tb["WB"])
    for ci in range(kw.get("n_dc_configs", 1)):
        e.set_dc_params(ci, p)
    e.assign(0, 0, 174, 188)
    e.reset()
    return e


@pytest.mark.parametrize("key,kw", [
    ("n_envs", dict(n=32)), ("episode_steps", dict(steps=24)), ("hist_cap", dict(hist_cap=5000)),
    ("queue_max_len", dict(queue_max_len=500)), ("max_roll_days", dict(max_roll_days=7)), ("n_locations", dict(n_locations=2)),
    ("n_dc_configs", dict(n_dc_configs=2)), ("env_index_base", dict(env_index_base=64)),
])
def test_load_refuses_a_checkpoint_of_another_shape(key, kw):
    import torch
    a = _small()
    a.step(torch.zeros((64, 3), dtype=torch.int32, device="cuda"))
    sd = a.state_dict()
    b = _small(**kw)
    with pytest.raises(ValueError, match=key):
        b.load_state_dict(sd)
    a.close()
    b.close()


def test_load_refuses_a_checkpoint_without_meta_or_of_another_layout():
    import copy
    a = _small()
    sd = a.state_dict()
    assert sd["meta"]["layout"] == a.lib.sdc_state_layout() and sd["meta"]["seed"] == 11
    old = {k: v for k, v in sd.items() if k != "meta"}
    with pytest.raises(ValueError, match="meta"):
        a.load_state_dict(old)
    bad = copy.deepcopy(sd)
    bad["meta"]["layout"] ^= 1
    with pytest.raises(ValueError, match="layout"):
        a.load_state_dict(bad)
    a.load_state_dict(sd)
    a.close()


def test_checkpoint_carries_the_seed_across_the_next_reset():
    """A's checkpoint loaded into an engine built with ANOTHER seed: the saved seed keys B's next resets, so B continues bit for
    bit with A across two episode boundaries (before the seed was part of the checkpoint, the next episode diverged)."""
    import torch
    a, b = _small(seed=11), _small(seed=99)
    g = torch.Generator(device="cpu").manual_seed(12)
    for t in range(10):
        a.step(_acts(64, g))
    a.set_seed(12345)                    # (a seed set after construction is the one that counts)
    b.load_state_dict(a.state_dict())
    assert b.seed == 12345
    ends = 0
    for t in range(40):
        x = _acts(64, g)
        ya = [v.clone() for v in a.step(x)]
        yb = b.step(x)
        for u, v, nm in zip(ya, yb, ("obs", "share_obs", "rew", "done", "info")):
            assert torch.equal(u, v), (t, nm)
        ends += int(ya[3].all())
    assert ends >= 2
    a.close()
    b.close()
