"""CPU tests of the Python binding's argument work (dc_rl_amd/_args.py and the pure functions of vec_env.py): every acceptance and
every refusal text of the validators, the output block's layout, the state-array table, the pair builders.  No GPU, no call into the
HIP library.  The expected texts and numbers are written out here: they are what the entry points said before the validators were
shared, not what the code under test computes."""
import numpy as np
import pytest
import torch

from dc_rl_amd import _args as A
from dc_rl_amd import _lib as L
from dc_rl_amd.vec_env import LOGGER_KEYS, keyed_sums, sel, sel_obs, share3_np, three_columns


def says(text, call, exc=ValueError):
    with pytest.raises(exc) as err:
        call()
    assert str(err.value) == text


# ---------------------------------------------------------------------------------------------------------------- index lists
def test_int_ids_accepts_and_refuses():
    for x in ([0, 3, 2], (0, 3, 2), np.array([0, 3, 2], dtype=np.int64), np.array([0, 3, 2], dtype=np.uint8), torch.tensor([0, 3, 2]),
              np.array([0, 3, 2, 9])[:3], np.array([0, 9, 3, 9, 2, 9])[::2]):
        a = A.int_ids(x, "snapshot: envs")
        assert a.dtype == np.int32 and a.flags.c_contiguous and a.tolist() == [0, 3, 2]
    s = A.int_ids(5, "restore: rows")
    assert s.ndim == 0 and s.dtype == np.int32 and int(s) == 5      # (a scalar stays 0-d: the pair builder broadcasts it)
    assert A.int_ids(np.int64(7), "restore: rows", 8).ndim == 0
    for empty in ([], np.zeros(0), np.zeros(0, dtype=np.float32), torch.zeros(0)):      # (an empty list is float64 to NumPy: accepted)
        a = A.int_ids(empty, "mark: envs")
        assert a.dtype == np.int32 and a.shape == (0,)
        assert A.int_ids(empty, "clone_envs: dst", 8).shape == (0,)
    assert A.int_ids([-2 ** 31, 2 ** 31 - 1], "mark: envs").tolist() == [-2 ** 31, 2 ** 31 - 1]
    assert A.int_ids([0, 7], "clone_envs: src", 8).tolist() == [0, 7]
    says("snapshot: envs must hold integers, got float64", lambda: A.int_ids([0.0, 1.0], "snapshot: envs"))
    says("mark: envs must hold integers, got float32", lambda: A.int_ids(torch.tensor([1.0]), "mark: envs"))
    says("rewind: envs must hold integers, got bool", lambda: A.int_ids([True], "rewind: envs"))
    says("restore: envs must hold integers, got <U1", lambda: A.int_ids(["0"], "restore: envs"))
    says("restore: rows must be one-dimensional, got shape (1, 2)", lambda: A.int_ids([[0, 1]], "restore: rows"))
    says("restore: rows holds a value outside int32", lambda: A.int_ids([0, 2 ** 31], "restore: rows"))
    says("restore: rows holds a value outside int32", lambda: A.int_ids([-2 ** 31 - 1], "restore: rows"))
    says("snapshot: envs holds a value outside int32", lambda: A.int_ids(2 ** 40, "snapshot: envs"))
    # with a range it is checked in place of the int32 bound
    says("clone_envs: dst holds an env index outside [0, 8)", lambda: A.int_ids([0, 8], "clone_envs: dst", 8))
    says("clone_envs: src holds an env index outside [0, 8)", lambda: A.int_ids(-1, "clone_envs: src", 8))
    says("clone_envs: src holds an env index outside [0, 8)", lambda: A.int_ids([2 ** 40], "clone_envs: src", 8))
    says("clone_envs: dst must hold integers, got float64", lambda: A.int_ids([1.5], "clone_envs: dst", 8))
    says("clone_envs: dst must be one-dimensional, got shape (2, 1)", lambda: A.int_ids([[0], [1]], "clone_envs: dst", 8))


def _pair(p, first, second):
    assert all(x.dtype == np.int32 and x.flags.c_contiguous and x.ndim == 1 for x in p)
    assert p[0].tolist() == first and p[1].tolist() == second


def test_clone_pairs():
    _pair(A.clone_pairs([0, 1], [2, 3], 8), [0, 1], [2, 3])
    _pair(A.clone_pairs(0, [2, 3, 4], 8), [0, 0, 0], [2, 3, 4])               # a scalar src is broadcast
    _pair(A.clone_pairs(np.int64(1), 7, 8), [1], [7])                           # ... a scalar dst is one destination
    _pair(A.clone_pairs(torch.tensor([5, 6]), torch.tensor([1, 2]), 8), [5, 6], [1, 2])
    _pair(A.clone_pairs(np.arange(8)[::2], np.arange(8)[1::2], 8), [0, 2, 4, 6], [1, 3, 5, 7])
    _pair(A.clone_pairs([], [], 8), [], [])                                    # (the library refuses an empty dst, in its own words)
    _pair(A.clone_pairs(0, np.zeros(0), 8), [], [])
    says("clone_envs: 2 sources for 3 destinations", lambda: A.clone_pairs([0, 1], [2, 3, 4], 8))
    says("clone_envs: 1 sources for 0 destinations", lambda: A.clone_pairs([0], [], 8))
    says("clone_envs: dst must hold integers, got float64", lambda: A.clone_pairs([0.5], [1.5], 8))      # dst is looked at first
    says("clone_envs: src must hold integers, got float64", lambda: A.clone_pairs([0.5], [1], 8))
    says("clone_envs: src must be one-dimensional, got shape (1, 2)", lambda: A.clone_pairs([[0, 1]], [2, 3], 8))
    says("clone_envs: src holds an env index outside [0, 8)", lambda: A.clone_pairs(2 ** 40, [1], 8))
    says("clone_envs: dst holds an env index outside [0, 8)", lambda: A.clone_pairs(0, [2 ** 40], 8))


def test_restore_pairs():
    snap = np.array([4, 5, 6], dtype=np.int32)
    _pair(A.restore_pairs(snap), [0, 1, 2], [4, 5, 6])                          # every row back where it came from
    _pair(A.restore_pairs(snap, [1, 2, 3]), [0, 1, 2], [1, 2, 3])
    _pair(A.restore_pairs(snap, [1, 2], [2, 0]), [2, 0], [1, 2])
    _pair(A.restore_pairs(snap, [0, 1, 2, 3], 1), [1, 1, 1, 1], [0, 1, 2, 3])   # a scalar row is broadcast
    _pair(A.restore_pairs(snap, rows=2), [2, 2, 2], [4, 5, 6])
    _pair(A.restore_pairs(snap, torch.tensor([7]), torch.tensor([0])), [0], [7])
    _pair(A.restore_pairs(snap, 7, 0), [0], [7])
    _pair(A.restore_pairs(snap, [], []), [], [])
    _pair(A.restore_pairs(snap, np.zeros(0), 1), [], [])
    _pair(A.restore_pairs(snap[:0]), [], [])
    says("restore: 2 envs for 3 snapshot rows: say which rows go where (rows=)", lambda: A.restore_pairs(snap, [0, 1]))
    says("restore: 2 rows for 3 envs", lambda: A.restore_pairs(snap, rows=[0, 1]))
    says("restore: 3 rows for 2 envs", lambda: A.restore_pairs(snap, [0, 1], [0, 1, 2]))
    says("restore: envs must hold integers, got float64", lambda: A.restore_pairs(snap, [0.5]))
    says("restore: rows must hold integers, got float64", lambda: A.restore_pairs(snap, rows=[0.5, 1, 2]))
    says("restore: envs must be one-dimensional, got shape (1, 3)", lambda: A.restore_pairs(snap, [[0, 1, 2]]))
    # restore holds its lists to int32 (the library checks the range), where clone_envs holds them to [0, n_envs)
    says("restore: rows holds a value outside int32", lambda: A.restore_pairs(snap, rows=[0, 1, 2 ** 40]))
    says("restore: envs holds a value outside int32", lambda: A.restore_pairs(snap, [0, 1, 2 ** 40]))


def test_group_sync_pairs():
    _pair(A.group_sync_pairs(2, 8, "n_envs"), [0, 2, 4, 6], [1, 3, 5, 7])
    _pair(A.group_sync_pairs(4, 8, "n_envs"), [0, 0, 0, 4, 4, 4], [1, 2, 3, 5, 6, 7])
    _pair(A.group_sync_pairs(8, 8, "num_envs"), [0] * 7, list(range(1, 8)))
    says("sync_groups: group_size = 1 must be at least 2 and divide n_envs = 8", lambda: A.group_sync_pairs(1, 8, "n_envs"))
    says("sync_groups: group_size = 3 must be at least 2 and divide num_envs = 8", lambda: A.group_sync_pairs(3, 8, "num_envs"))
    says("sync_groups: group_size = 16 must be at least 2 and divide n_envs = 8", lambda: A.group_sync_pairs(16, 8, "n_envs"))
    from dc_rl_amd import engine
    assert engine.group_sync_pairs is A.group_sync_pairs and engine._STATE_DTYPES is A.STATE_SCALARS


# ---------------------------------------------------------------------------------------------------------------- tensors, horizons
def test_device_tensor_texts():
    """(a CPU tensor is refused whatever else it is: the acceptances and the is-on-another-device text need a GPU --
    tests/test_gpu_engine_refusals.py)"""
    x = torch.zeros((2, 8, 3), dtype=torch.int32)
    says("actions must be a contiguous int32 CUDA tensor of shape (K, n_envs, 3)",
         lambda: A.device_tensor(x, "", "actions", torch.int32, (A.ANY, 8, 3), "(K, n_envs, 3)"))
    says("rollout_stats: actions must be a contiguous int32 CUDA tensor of shape (K, n_envs, 3)",
         lambda: A.device_tensor(x, "rollout_stats", "actions", torch.int32, (A.ANY, 8, 3), "(K, n_envs, 3)", torch.device("cuda", 0), True))
    for who in ("lookahead", "plan"):
        says(f"{who}: actions must be a contiguous int32 CUDA tensor of shape (M, K, n_envs, 3)",
             lambda: A.device_tensor(x[None], who, "actions", torch.int32, (A.SOME, A.SOME, 8, 3), "(M, K, n_envs, 3)"))
    says("plan_cem: probs must be a contiguous float64 CUDA tensor of shape (4, 8, 3, 3)",
         lambda: A.device_tensor(None, "plan_cem", "probs", torch.float64, (4, 8, 3, 3)))
    says("plan_cem_groups: best_seq must be a contiguous int32 CUDA tensor of shape (4, 2, 3)",
         lambda: A.device_tensor(x.numpy(), "plan_cem_groups", "best_seq", torch.int32, (4, 2, 3)))


def test_is_tensor_patterns_on_the_host():
    x = torch.zeros((2, 8, 3), dtype=torch.int32)
    ok = lambda t, shape, dtype=torch.int32, **kw: A.is_tensor(t, dtype, shape, cuda=False, **kw)
    assert ok(x, (2, 8, 3)) and ok(x, (A.ANY, 8, 3)) and ok(x, (A.SOME, 8, 3)) and ok(x[:0], (A.ANY, 8, 3))
    assert ok(x, (2, 8, 3), device=torch.device("cpu"))
    assert not ok(x[:0], (A.SOME, 8, 3)) and not ok(x, (2, 8)) and not ok(x, (2, 8, 3, 1)) and not ok(x, (2, 7, 3))
    assert not ok(x, (2, 8, 3), torch.int64) and not ok(x[:, ::2], (2, 4, 3)) and not ok(x.numpy(), (2, 8, 3)) and not ok(None, ())
    assert not ok(x, (2, 8, 3), device=torch.device("cuda", 0)) and not A.is_tensor(x, torch.int32, (2, 8, 3))


def test_horizon_rules():
    A.check_horizon("plan", 256)
    A.check_horizon("lookahead", 5, left=6, auto_reset=True)
    A.check_horizon("lookahead", 6, left=6, auto_reset=False)
    says("plan: K = 257 is more than a mark holds (MARK_MAX_STEPS = 256)", lambda: A.check_horizon("plan", 257))
    says("lookahead: K = 257 is more than a mark holds (MARK_MAX_STEPS = 256)", lambda: A.check_horizon("lookahead", 257, 1, True))
    says("lookahead: K = 6 steps would finish an episode (6 steps left): the auto-reset kills the mark",
         lambda: A.check_horizon("lookahead", 6, 6, True))
    says("lookahead: K = 7 steps would finish an episode (6 steps left): the auto-reset kills the mark",
         lambda: A.check_horizon("lookahead", 7, 6, True))
    says("lookahead: K = 7 steps would run past the end of an episode (6 steps left)", lambda: A.check_horizon("lookahead", 7, 6, False))


# ---------------------------------------------------------------------------------------------------------------- the output block
@pytest.mark.parametrize("N", [1, 3, 64])
def test_output_layout(N):
    blocks, nbytes = A.out_layout(N)
    # obs 3 x 26, share_obs 29, rew 3, info 44 floats per env, in that order; then one done byte per env
    a = N * 3 * 26
    b = a + N * 29
    c = b + N * 3
    n_f = N * (3 * 26 + 29 + 3 + 44)
    assert blocks == [("obs", "float32", (N, 3, 26), 0), ("share", "float32", (N, 29), a), ("rew", "float32", (N, 3), b),
                      ("info", "float32", (N, 44), c), ("done", "uint8", (N,), n_f)]
    assert nbytes == n_f * 4 + N == 617 * N
    flat = torch.arange(nbytes, dtype=torch.int64).to(torch.uint8)
    v = A.out_views(flat, N)
    assert list(v) == ["obs", "share", "rew", "info", "done"]
    at = 0      # the five views tile the block: each starts where the one before ends, done last
    for name, dtype, shape, _ in blocks:
        x = v[name]
        assert x.dtype == getattr(torch, dtype) and tuple(x.shape) == shape and x.is_contiguous()
        assert x.data_ptr() == flat.data_ptr() + at, name
        at += x.numel() * x.element_size()
    assert at == nbytes == flat.numel()
    for x in v.values():      # ... and are views, not copies
        x.view(torch.uint8).zero_()
    assert not flat.any()


# ---------------------------------------------------------------------------------------------------------------- state arrays
def test_state_array_table():
    sizes = dict(n_envs=5, hist_stride=10016, lw=200, queue_stride=1008, hist_cap=10000)
    i32, u32, f32, f64 = np.int32, np.uint32, np.float32, np.float64
    want = {"cursor": (i32, (5,)), "t_rel": (i32, (5,)), "day": (i32, (5,)), "hourq": (i32, (5,)), "q_popped": (i32, (5,)),
            "q_cum": (i32, (5,)), "q_cumT": (u32, (5,)), "q_head": (i32, (5,)), "q_cum_hm1": (i32, (5,)), "q_cumT_hm1": (u32, (5,)),
            "last_delta": (i32, (5,)), "consecutive": (i32, (5,)), "scale": (i32, (5,)), "hist_len": (i32, (5,)), "hist_pos": (i32, (5,)),
            "episode": (i32, (5,)), "fault": (u32, (5,)), "loc_id": (i32, (5,)), "cfg_id": (i32, (5,)), "day_lo": (i32, (5,)),
            "day_hi": (i32, (5,)), "hist_n": (i32, (5,)), "order_stat_sticky": (u32, (5,)), "stpt": (f64, (5,)), "bat_load": (f64, (5,)),
            "ci_min": (f64, (5,)), "ci_den": (f64, (5,)), "t_min": (f64, (5,)), "t_den": (f64, (5,)), "hist_ref": (f64, (5,)),
            "hist": (f32, (5, 10016)), "t_win": (f64, (5, 200)), "wb_win": (f64, (5, 200)), "qtab": (u32, (5, 1008, 2)),
            "qcum_t": (u32, (1008, 5)), "hist_t": (u32, (10000, 5)), "record": (u32, (5, 64)), "ep_return": (f64, (5, 3)),
            "header": (u32, (5, 64)), "qwin": (u32, (5, 64, 4))}
    assert set(A.STATE_ARRAYS) == set(want) and len(A.STATE_SCALARS) == 30
    for name, (dt, shape) in want.items():
        a = A.state_array(name, sizes)
        assert a.dtype == dt and a.shape == shape and a.flags.c_contiguous and not a.any(), name
    says("'no_such_state'", lambda: A.state_array("no_such_state", sizes), KeyError)


# ---------------------------------------------------------------------------------------------------------------- reset overrides
def test_reset_override_table():
    sizes = dict(n_envs=4, lw=10)
    i, f = (lambda v, n=4: np.full(n, v, dtype=np.int64)), (lambda v, n=4: np.full(n, v, dtype=np.float32))
    good = dict(day=i(180), hour=i(3), ci_min=f(1), ci_max=f(2), t_min=f(3), t_max=f(4), t_win=np.ones((4, 10)), wb_win=np.ones((4, 10)))
    a = A.reset_override(good, sizes)
    assert list(a) == ["day", "hour", "ci_min", "ci_max", "t_min", "t_max", "t_win", "wb_win"]      # sdc_reset_override's fields
    assert all(x.flags.c_contiguous for x in a.values()) and {k: x.dtype for k, x in a.items()} == dict(
        day=np.int32, hour=np.int32, ci_min=np.float64, ci_max=np.float64, t_min=np.float64, t_max=np.float64, t_win=np.float64,
        wb_win=np.float64)
    for k in ("day", "hour", "ci_min", "ci_max", "t_min", "t_max"):
        says("override scalars must have shape (n_envs,)", lambda: A.reset_override(dict(good, **{k: good[k][:3]}), sizes))
    says("override scalars must have shape (n_envs,)", lambda: A.reset_override(dict(good, day=i(1, 3), t_win=np.ones((4, 9))), sizes))
    for k in ("t_win", "wb_win"):
        says("override weather windows must have shape (4, 10)", lambda: A.reset_override(dict(good, **{k: np.ones((4, 9))}), sizes))
    with pytest.raises(KeyError):
        A.reset_override({k: v for k, v in good.items() if k != "t_max"}, sizes)
    noise = dict(day=i(180), hour=i(3), roll_days=i(0), noise=np.zeros((4, L.TABLE_LEN), dtype=np.float32))
    a = A.reset_override(noise, sizes)
    assert list(a) == ["day", "hour", "roll_days", "noise"] and a["noise"].dtype == np.float64 and a["roll_days"].dtype == np.int32
    for k, x in (("day", i(1, 3)), ("roll_days", i(0, 5)), ("noise", np.zeros((4, 35039))), ("noise", np.zeros(35040))):
        says("noise injection: noise (4, 35040), day / hour / roll_days (4,)", lambda: A.reset_override(dict(noise, **{k: x}), sizes))
    assert {f for f, _ in L.SdcResetOverride._fields_} == {f for kind in A.RESET_OVERRIDES.values() for f, _, _ in kind}


# ---------------------------------------------------------------------------------------------------------------- the vector env's
def test_three_columns():
    dev = torch.device("cpu")
    a = torch.tensor([[0, 1, 2], [2, 1, 0]], dtype=torch.int64)
    full = three_columns(a, [0, 1, 2], dev)
    assert full.dtype == torch.int32 and full.is_contiguous() and full.tolist() == [[0, 1, 2], [2, 1, 0]]
    b = torch.tensor([[0, 1, 2], [2, 1, 0]], dtype=torch.int32)
    assert three_columns(b, [0, 1, 2], dev) is b                       # already the engine's: handed on, not copied
    assert not three_columns(b.t(), [0, 1, 2], dev).t().is_contiguous() and three_columns(b.t(), [0, 1, 2], dev).is_contiguous()
    # an agent subset: the other slots' columns are filled with 1
    assert three_columns(torch.tensor([[0, 2], [2, 0]]), [1, 2], dev).tolist() == [[1, 0, 2], [1, 2, 0]]
    assert three_columns(torch.tensor([[0], [2]]), [1], dev).tolist() == [[1, 0, 1], [1, 2, 1]]
    seq = three_columns(torch.tensor([[[[0, 2]], [[2, 0]]]]), [0, 2], dev)                      # [M, K, N, n_agents]
    assert seq.shape == (1, 2, 1, 3) and seq.tolist() == [[[[0, 1, 2]], [[2, 1, 0]]]]
    # step_async's form: the runners' [N, n_agents, 1] goes through reshape(N, n_agents) first
    assert three_columns(torch.tensor([[[0], [2]], [[2], [0]]]).reshape(2, 2), [1, 2], dev).tolist() == [[1, 0, 2], [1, 2, 0]]


def test_keyed_sums():
    assert keyed_sums(["dc_water_usage", "ls_unasigned_day_load_left", "bat_SOC"], np.array([2.5, 7.0])) == {
        "dc_water_usage": 2.5, "ls_unasigned_day_load_left": 0.0, "bat_SOC": 7.0}      # a key that is no column: constant 0
    out = keyed_sums(LOGGER_KEYS, np.arange(9, dtype=np.float64))
    assert list(out) == list(LOGGER_KEYS) and all(type(v) is float for v in out.values())
    assert out["ls_unasigned_day_load_left"] == 0.0 and out["dc_HVAC_total_power_kW"] == 8.0 and out["ls_tasks_in_queue"] == 3.0
    assert keyed_sums([], np.zeros(0)) == {}


def test_agent_selection_and_shared_observation():
    obs = np.arange(2 * 3 * 26, dtype=np.float32).reshape(2, 3, 26)
    share = np.arange(2 * 29, dtype=np.float32).reshape(2, 29)
    assert sel(obs, [0, 1, 2]) is obs and sel_obs(obs, [0, 1, 2], 26) is obs
    assert np.array_equal(sel(obs, [1, 2]), obs[:, 1:]) and np.array_equal(sel_obs(obs, [1, 2], 14), obs[:, 1:, :14])
    s = share3_np(share, obs, [0, 1, 2], 26, False)
    assert s.shape == (2, 3, 29) and all(np.array_equal(s[:, a], share) for a in range(3))
    s = share3_np(share, obs, [1, 2], 14, True)      # the trained agents' padded observations, concatenated
    assert s.shape == (2, 2, 28) and np.array_equal(s[:, 1], np.concatenate([obs[:, 1, :14], obs[:, 2, :14]], axis=1))
    t = torch.from_numpy(obs)
    assert sel(t, [0, 1, 2]) is t and torch.equal(sel_obs(t, [2], 13), t[:, 2:, :13])
