"""What the Python binding itself refuses, through public methods only: for every entry point that takes tensors, index lists or a
horizon, each malformed argument raises the exception type and the FULL text written here (literals: the texts are the interface), and
leaves the engine as it was (its `record` state to the bit).  One acceptance per entry point with the smallest legal arguments shows
that good input passes; a rollout on a pinned stream gives the bits of one on torch's current stream.  8 envs, episodes of the default
672 steps, one engine and one vector env for the module."""
import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import SustainDCVecEnv
from dc_rl_amd.engine import EnvMark, EnvSnapshot, EpisodeStats
from tests.test_gpu_mark import _mk

pytestmark = pytest.mark.gpu
N, HISTORY = 8, 500      # (500 steps in: 172 left, fewer than a mark holds -- the episode-end rule is in reach)
RSV = L.INFO_IDX["reserved"]


@pytest.fixture(scope="module")
def eng():
    e = _mk(N, ep=672)
    e.rollout(_seq(HISTORY))
    yield e
    e.close()


@pytest.fixture(scope="module")
def venv():
    v = SustainDCVecEnv({"location": "ny", "month": 6, "partial_obs": True, "nonoverlapping_shared_obs_space": True}, n_envs=N, seed=3,
                        return_torch=True)
    yield v
    v.close()


def _seq(*lead, last=3, dtype=None, seed=0):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 3, lead + (N, last), dtype=torch.int32, generator=g).to(dtype or torch.int32).cuda()


class _NotStats:
    def __init__(self, res):
        self.stats, self.returns, self.counts = res.stats, res.returns, res.counts


def refused(engine, exc, text, call):
    before = engine.get_state("record")
    with pytest.raises(exc) as err:
        call()
    assert str(err.value) == text
    assert np.array_equal(before, engine.get_state("record")), text


def malformed(*lead):
    """action tensors that are not a contiguous int32 CUDA tensor of shape lead + (N, 3): what is wrong -> the tensor"""
    import torch
    return {"dtype": _seq(*lead, dtype=torch.int64), "rank": _seq(*lead)[0], "agents": _seq(*lead, last=2),
            "envs": _seq(*lead)[..., :N - 1, :].contiguous(), "strides": _seq(*lead, last=6)[..., ::2], "host": _seq(*lead).cpu(),
            "type": _seq(*lead).cpu().numpy()}


# ---------------------------------------------------------------------------------------------------------------- the engine
def test_rollout(eng):
    for what, x in malformed(2).items():
        refused(eng, ValueError, "actions must be a contiguous int32 CUDA tensor of shape (K, n_envs, 3)", lambda: eng.rollout(x))
    refused(eng, ValueError, "n_steps does not match the action sequence", lambda: eng.rollout(_seq(2), n_steps=3))
    refused(eng, ValueError, "actions=None needs n_steps and a built-in policy on every agent slot", lambda: eng.rollout(None, n_steps=2))
    left = eng.steps_to_episode_end()
    obs, share, rew, done, info = eng.rollout(_seq(1))
    assert obs.shape == (1, N, 3, 26) and info.shape == (1, N, 44) and eng.steps_to_episode_end() == left - 1


def test_rollout_on_a_pinned_stream_gives_the_same_bits(eng):
    import torch
    acts = _seq(4, seed=1)
    mk = eng.mark(max_steps=4)
    plain = eng.rollout(acts, want_actions=True)
    eng.rewind(mk)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    eng.use_stream(s)
    try:
        pinned = eng.rollout(acts, want_actions=True)
        s.synchronize()
    finally:
        eng.use_stream(None)
    for nm, u, v in zip(("obs", "share_obs", "rew", "done", "info", "actions"), plain, pinned):
        if nm == "info":      # (the diagnostics column says how the reward state was served: a rewind clears the stamps it follows)
            u, v = u.clone(), v.clone()
            u[..., RSV] = 0
            v[..., RSV] = 0
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), nm
    eng.rewind(mk)


def test_rollout_stats(eng):
    import torch
    for what, x in malformed(2).items():
        refused(eng, ValueError, "rollout_stats: actions must be a contiguous int32 CUDA tensor of shape (K, n_envs, 3)",
                lambda: eng.rollout_stats(x))
    refused(eng, ValueError, "rollout_stats: n_steps does not match the action sequence", lambda: eng.rollout_stats(_seq(2), n_steps=3))
    refused(eng, ValueError, "rollout_stats: actions=None needs n_steps and a built-in policy on every agent slot",
            lambda: eng.rollout_stats(None, n_steps=2))
    res = eng.rollout_stats(_seq(1))
    assert res.stats.shape == (4, N, 44) and (res.steps == 1).all()
    text = ("rollout_stats: into must be an EpisodeStats of this engine (contiguous tensors on cuda:0: stats float64 (4, 8, 44), returns "
            "float64 (8, 3), counts int32 (8, 2))")
    for into in (EpisodeStats(res.stats.float(), res.returns, res.counts), EpisodeStats(res.stats, res.returns[:, :2], res.counts),
                 EpisodeStats(res.stats, res.returns, res.counts.t().contiguous().t()),
                 EpisodeStats(res.stats.cpu(), res.returns.cpu(), res.counts.cpu()), _NotStats(res)):
        refused(eng, ValueError, text, lambda: eng.rollout_stats(_seq(1), into=into))
    assert eng.rollout_stats(_seq(1), into=res) is res and (res.steps == 2).all()


def test_lookahead_and_plan(eng):
    left = eng.steps_to_episode_end()
    assert 2 < left <= L.MARK_MAX_STEPS
    for who, call in (("lookahead", eng.lookahead), ("plan", eng.plan)):
        bad = dict(malformed(2, 2), no_candidate=_seq(0, 2), no_step=_seq(2, 0))
        for what, x in bad.items():
            refused(eng, ValueError, f"{who}: actions must be a contiguous int32 CUDA tensor of shape (M, K, n_envs, 3)", lambda: call(x))
        refused(eng, ValueError, f"{who}: K = 257 is more than a mark holds (MARK_MAX_STEPS = 256)", lambda: call(_seq(1, 257)))
    refused(eng, ValueError, f"lookahead: K = {left} steps would finish an episode ({left} steps left): the auto-reset kills the mark",
            lambda: eng.lookahead(_seq(1, left)))
    refused(eng, ValueError, "plan: reward_weights must be three numbers (ls, dc, bat), got 2",
            lambda: eng.plan(_seq(2, 1), reward_weights=(1.0, 1.0)))
    refused(eng, ValueError, "plan: info_weights key 'no_such_key' is not an info column (dc_rl_amd._lib.INFO_COLS)",
            lambda: eng.plan(_seq(2, 1), info_weights={"no_such_key": 1.0}))
    refused(eng, ValueError, "plan: info_weights names 9 keys, at most 8 can be weighed",
            lambda: eng.plan(_seq(2, 1), info_weights={k: 1.0 for k in L.INFO_COLS[:9]}))
    a = _seq(2, 1)
    ret, res = eng.lookahead(a), eng.plan(a)
    assert ret.shape == (2, N, 3) and res.returns.shape == (2, N, 3) and res.action.shape == (N, 3) and res.score.shape == (2, N)
    assert (ret == res.returns).all() and eng.steps_to_episode_end() == left


def test_plan_cem_and_plan_cem_groups(eng):
    import torch
    left = eng.steps_to_episode_end()
    for who, lead, call in (("plan_cem", N, lambda **kw: eng.plan_cem(2, 1, 2, 1, **kw)),
                            ("plan_cem_groups", N // 2, lambda **kw: eng.plan_cem_groups(2, 2, 1, 1, **kw))):
        refused(eng, ValueError, f"{who}: fixed_action must be three integers (ls, dc, bat), got 2", lambda: call(fixed_action=(1, 1)))
        for kw in (dict(seed=-1), dict(seed=1 << 64), dict(draw=-1), dict(draw=1 << 32)):
            refused(eng, ValueError, f"{who}: seed must fit 64 bits and draw 32, both unsigned", lambda: call(**kw))
        p = torch.full((2, lead, 3, 3), 1.0 / 3.0, dtype=torch.float64, device="cuda")
        b = torch.ones((2, lead, 3), dtype=torch.int32, device="cuda")
        for x in (p.float(), p[0], p[:, :-1].contiguous(), p.transpose(2, 3), p.cpu(), p.cpu().numpy()):
            refused(eng, ValueError, f"{who}: probs must be a contiguous float64 CUDA tensor of shape (2, {lead}, 3, 3)", lambda: call(probs=x))
        for x in (b.long(), b[0], b[:, :-1].contiguous(), torch.ones((2, lead, 6), dtype=torch.int32, device="cuda")[..., ::2], b.cpu()):
            refused(eng, ValueError, f"{who}: best_seq must be a contiguous int32 CUDA tensor of shape (2, {lead}, 3)", lambda: call(best_seq=x))
        refused(eng, ValueError, "plan: reward_weights must be three numbers (ls, dc, bat), got 2", lambda: call(reward_weights=(1.0, 1.0)))
    refused(eng, ValueError, "plan_cem_groups: group_base must fit 32 bits", lambda: eng.plan_cem_groups(2, 1, 1, 1, group_base=1 << 31))
    res = eng.plan_cem(1, 1, 2, 1)
    assert res.action.shape == (N, 3) and res.cand.shape == (2, 1, N, 3) and res.best_score.shape == (1, N)
    eng.sync_groups(2)
    res = eng.plan_cem_groups(2, 1, 1, 1)
    assert res.action.shape == (N // 2, 3) and res.step_actions.shape == (N, 3) and res.cand.shape == (1, N, 3)
    assert eng.steps_to_episode_end() == left


def test_clone_envs(eng):
    refused(eng, ValueError, "clone_envs: dst must hold integers, got float64", lambda: eng.clone_envs([0], [1.0]))
    refused(eng, ValueError, "clone_envs: src must hold integers, got float64", lambda: eng.clone_envs([0.5], [1]))
    refused(eng, ValueError, "clone_envs: src must be one-dimensional, got shape (1, 2)", lambda: eng.clone_envs([[0, 1]], [2, 3]))
    refused(eng, ValueError, "clone_envs: dst holds an env index outside [0, 8)", lambda: eng.clone_envs([0], [8]))
    refused(eng, ValueError, "clone_envs: src holds an env index outside [0, 8)", lambda: eng.clone_envs([-1], [1]))
    refused(eng, ValueError, "clone_envs: 2 sources for 3 destinations", lambda: eng.clone_envs([0, 1], [2, 3, 4]))
    import torch
    obs, share = eng.clone_envs(0, 1)
    assert obs is eng.obs and share is eng.share_obs and torch.equal(obs[0], obs[1]) and torch.equal(share[0], share[1])


def test_snapshot_and_restore(eng):
    import torch
    refused(eng, ValueError, "snapshot: envs must hold integers, got float64", lambda: eng.snapshot([0.5]))
    refused(eng, ValueError, "snapshot: envs must be one-dimensional, got shape (1, 2)", lambda: eng.snapshot([[0, 1]]))
    refused(eng, ValueError, "snapshot: envs holds a value outside int32", lambda: eng.snapshot([2 ** 40]))
    assert len(eng.snapshot([0])) == 1
    snap = eng.snapshot([0, 1, 2])
    rb = int(snap.rows.shape[1])
    refused(eng, ValueError, "restore: envs must hold integers, got float64", lambda: eng.restore(snap, [0.0, 1.0, 2.0]))
    refused(eng, ValueError, "restore: rows must hold integers, got float64", lambda: eng.restore(snap, rows=[0.0, 1.0, 2.0]))
    refused(eng, ValueError, "restore: rows must be one-dimensional, got shape (1, 3)", lambda: eng.restore(snap, rows=[[0, 1, 2]]))
    refused(eng, ValueError, "restore: rows holds a value outside int32", lambda: eng.restore(snap, rows=[0, 1, 2 ** 40]))
    refused(eng, ValueError, "restore: 2 envs for 3 snapshot rows: say which rows go where (rows=)", lambda: eng.restore(snap, [3, 4]))
    refused(eng, ValueError, "restore: 2 rows for 3 envs", lambda: eng.restore(snap, rows=[0, 1]))
    other = lambda **kw: EnvSnapshot(kw.get("rows", snap.rows), kw.get("manifest", snap.manifest), kw.get("meta", snap.meta), snap.envs)
    refused(eng, ValueError, "restore: manifest of shape (2, 9) for 3 rows", lambda: eng.restore(other(manifest=snap.manifest[:2])))
    refused(eng, ValueError, "restore: manifest of shape (27,) for 3 rows", lambda: eng.restore(other(manifest=snap.manifest.reshape(-1))))
    refused(eng, ValueError, f"restore: rows must be a contiguous uint8 tensor [n, {rb}], got (3, {rb})",
            lambda: eng.restore(other(rows=snap.rows.to(torch.int32))))
    refused(eng, ValueError, f"restore: rows must be a contiguous uint8 tensor [n, {rb}], got (3, {rb - 1})",
            lambda: eng.restore(other(rows=snap.rows[:, :-1].contiguous())))
    refused(eng, ValueError, f"restore: rows must be a contiguous uint8 tensor [n, {rb}], got ({3 * rb},)",
            lambda: eng.restore(other(rows=snap.rows.reshape(-1))))
    refused(eng, ValueError, "restore: the snapshot's rows are on cpu, this engine runs on cuda:0 (snapshot.to(device))",
            lambda: eng.restore(snap.to("cpu")))
    refused(eng, ValueError, "restore: snapshot episode_steps = 96, this engine's is 672",
            lambda: eng.restore(other(meta=dict(snap.meta, episode_steps=96))))
    left = eng.steps_to_episode_end()
    obs, share = eng.restore(snap)
    assert obs is eng.obs and share is eng.share_obs and eng.steps_to_episode_end() == left


def test_mark_and_rewind(eng):
    for K in (0, -1, 257):
        refused(eng, ValueError, f"mark: max_steps = {K} outside [1, 256]", lambda: eng.mark(max_steps=K))
    refused(eng, ValueError, "mark: envs must hold integers, got float64", lambda: eng.mark([0.5]))
    refused(eng, ValueError, "mark: envs must be one-dimensional, got shape (1, 2)", lambda: eng.mark([[0, 1]]))
    refused(eng, ValueError, "mark: envs holds a value outside int32", lambda: eng.mark([-2 ** 40]))
    mk = eng.mark([0, 1], max_steps=1)
    refused(eng, ValueError, "rewind: not an EnvMark", lambda: eng.rewind(None))
    refused(eng, ValueError, "rewind: envs must hold integers, got float64", lambda: eng.rewind(mk, [0.0]))
    refused(eng, ValueError, "rewind: envs must be one-dimensional, got shape (1, 2)", lambda: eng.rewind(mk, [[0, 1]]))
    refused(eng, ValueError, "rewind: env 5 is not one of the mark's envs", lambda: eng.rewind(mk, [0, 5]))
    refused(eng, ValueError, "rewind: no env", lambda: eng.rewind(mk, []))
    refused(eng, ValueError, "rewind: the mark's rows are on cpu, this engine runs on cuda:0",
            lambda: eng.rewind(EnvMark(mk.rows.cpu(), mk.manifest, mk.envs, 1, False)))
    before = eng.get_state("record")
    whole = eng.mark(max_steps=1)
    assert len(whole) == N and whole.whole
    eng.rollout(_seq(1))
    obs, share = eng.rewind(whole)
    assert obs is eng.obs and np.array_equal(before, eng.get_state("record"))


def test_reset_override(eng):
    """(last of the engine's tests: the acceptance starts a new episode)"""
    from dc_rl_amd import traces
    day = traces.get_init_day(6)      # (the middle of the days the engine's envs are assigned)
    i, f = (lambda v: np.full(N, v, dtype=np.int32)), (lambda v: np.full(N, v, dtype=np.float64))
    win = lambda v, n=N: np.full((n, eng.lw), v, dtype=np.float64)
    good = dict(day=i(day), hour=i(3), ci_min=f(100.0), ci_max=f(500.0), t_min=f(-10.0), t_max=f(40.0), t_win=win(20.0), wb_win=win(15.0))
    refused(eng, ValueError, "mask must have shape (n_envs,)", lambda: eng.reset(mask=np.ones(N - 1, dtype=np.uint8)))
    for k in ("day", "hour", "ci_min", "ci_max", "t_min", "t_max"):
        refused(eng, ValueError, "override scalars must have shape (n_envs,)", lambda: eng.reset(override=dict(good, **{k: good[k][:-1]})))
    for k in ("t_win", "wb_win"):
        for x in (win(20.0, N - 1), win(20.0)[:, :-1], win(20.0).reshape(-1)):
            refused(eng, ValueError, f"override weather windows must have shape (8, {eng.lw})",
                    lambda: eng.reset(override=dict(good, **{k: x})))
    noise = dict(day=i(day), hour=i(3), roll_days=i(0), noise=np.zeros((N, L.TABLE_LEN)))
    for k, x in (("day", i(day)[:-1]), ("hour", i(3)[:-1]), ("roll_days", np.zeros((N, 1), dtype=np.int32)),
                 ("noise", np.zeros((N, L.TABLE_LEN - 1))), ("noise", np.zeros((N - 1, L.TABLE_LEN)))):
        refused(eng, ValueError, "noise injection: noise (8, 35040), day / hour / roll_days (8,)",
                lambda: eng.reset(override=dict(noise, **{k: x})))
    obs, share = eng.reset(override=good)
    assert obs is eng.obs and share is eng.share_obs and eng.steps_to_episode_end() == 672


# ---------------------------------------------------------------------------------------------------------------- the vector env
def test_vec_env_before_reset(venv):
    calls = {"clone_envs": lambda: venv.clone_envs(0, 1), "snapshot": venv.snapshot, "restore": lambda: venv.restore(None),
             "mark": venv.mark, "rewind": lambda: venv.rewind(None), "plan": lambda: venv.plan(None),
             "plan_cem": lambda: venv.plan_cem(1, 1, 2, 1), "plan_cem_groups": lambda: venv.plan_cem_groups(2, 1, 1, 1),
             "rollout_stats": lambda: venv.rollout_stats(n_steps=1)}
    for name, call in calls.items():
        refused(venv.engine, ValueError, f"{name}: call reset() first", call)
    refused(venv.engine, ValueError, "clone_envs: call reset() first", lambda: venv.sync_groups(2))


def test_vec_env_shapes_and_acceptances(venv):
    import torch
    e = venv.engine
    obs, share, avail = venv.reset()
    assert obs.shape == (N, 3, 26) and share.shape == (N, 3, 29) and avail.shape == (N, 3, 3)
    for x in (_seq(2, 1)[0], _seq(2, 1, last=2), _seq(2, 1)[:, :, :N - 1], _seq(2, 1).cpu().numpy()):
        refused(e, ValueError, "plan: actions must be a tensor of shape (M, K, 8, 3)", lambda: venv.plan(x))
    for x in (_seq(1)[0], _seq(1, last=2), _seq(1)[:, :N - 1], _seq(1).cpu().numpy()):
        refused(e, ValueError, "rollout_stats: actions must be a tensor of shape (K, 8, 3)", lambda: venv.rollout_stats(x))
        refused(e, ValueError, "evaluate: actions must be a tensor of shape (K, 8, 3)", lambda: venv.evaluate(1, x))
    refused(e, ValueError, "rollout_stats: actions=None needs n_steps", venv.rollout_stats)
    refused(e, ValueError, "rollout_stats: n_steps does not match the action sequence", lambda: venv.rollout_stats(_seq(2), n_steps=3))
    refused(e, ValueError, "evaluate: actions must hold episode_steps = 672 steps, got 2", lambda: venv.evaluate(1, _seq(2)))
    refused(e, ValueError, "sync_groups: group_size = 3 must be at least 2 and divide num_envs = 8", lambda: venv.sync_groups(3))
    snap = venv.snapshot([0, 1])
    foreign = EnvSnapshot(snap.rows, snap.manifest, snap.meta, snap.envs)
    refused(e, ValueError, "restore: the snapshot was not taken from a vector env with these data-centre configs and trace sets",
            lambda: venv.restore(foreign))
    # the smallest legal call of each; the host-side layers hand their arguments on in the engine's shapes
    triple = lambda r: r[0].shape == (N, 3, 26) and r[1].shape == (N, 3, 29) and r[2].shape == (N, 3, 3)
    assert triple(venv.clone_envs(0, 1)) and triple(venv.restore(snap)) and triple(venv.sync_groups(2))
    mk = venv.mark(max_steps=1)
    venv.step(_seq())
    assert triple(venv.rewind(mk))
    assert venv.plan(_seq(2, 1).long()).action.shape == (N, 3)
    assert venv.plan_cem(1, 1, 2, 1).action.shape == (N, 3)
    assert venv.plan_cem_groups(2, 1, 1, 1).step_actions.shape == (N, 3)
    assert (venv.rollout_stats(_seq(1)).steps == 1).all()
    o, s, r, d, infos, a = venv.step(_seq().view(N, 3, 1))      # ([N, n_agents, 1]: the runners' action shape)
    assert o.shape == (N, 3, 26) and r.shape == (N, 3, 1) and d.shape == (N, 3)
    assert infos[0][0]["ls_action"] in (0, 1, 2)
