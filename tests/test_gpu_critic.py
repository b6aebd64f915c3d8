"""The V critic on the device (sdc_set_critic / sdc_critic_values / sdc_set_plan_critic; csrc/sdc_critic.hpp) held to the restatement
of the reference's VNet + ValueNorm in tests/critic_ref.py (torch fp64) and to the header's contract (include/sustaindc_hip.h THE
CRITIC):

 1. values against the restatement within 2e-4 * scale (the bound tests/test_gpu_actor.py holds the same depth and widths to) -- row
    counts 1, 15, 16, 17, 63, 64, 65 and a [5, 40, 29] tensor, real share_obs rows and Gaussian rows, tanh / relu x feature LayerNorm on /
    off x ValueNorm on / off; torch fp32's own distance from fp64 is printed next to the observed maximum;  2. a dead ReLU layer (the
    variance-0 path);  3. a row's value depends on that row alone: reversed order, a shorter call, nothing stored past the last row;
 4. `plan` with the critic as terminal value: score_w - score_0 = gamma^K * w * V * (1 - done) per candidate and env, V from a third
    twin's materialised rollout; returns untouched; best the first maximum; also four envs per wavefront and with the horizon in two
    chunks;  5. the term is exactly 0 where the horizon ends the episode;  6. plan_cem and plan_cem_groups;  7. weight 0 after a weight
    is a plan that never saw a critic;  8. rollout_actor(want_values=True);  9. copy.deepcopy of a SustainDCVecEnv;  10. the refusals.

One small engine as in tests/test_gpu_actor.py for the values; the planners' twins are tests/plan_util.py's (episodes of 96 steps)."""
import copy
import ctypes as C

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import SustainDCVecEnv
from tests import critic_ref as CR
from tests.actor_ref import engine as small_engine
from tests.plan_util import _twins, refused
from tests.test_gpu_mark import _mk
from tests.test_gpu_plan import _cands

pytestmark = pytest.mark.gpu

BOUND = 2e-4
ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65)
W, GAMMA, WEIGHT = (0.5, 2.0, -1.0), 0.9, 0.5
COLS = {"bat_CO2_footprint": -1e-3, "energy_z": 3.0}
OBJ = dict(reward_weights=W, gamma=GAMMA, info_weights=COLS)
CRITIC_KERNELS = ("sdc_critic_values_kernel", "sdc_critic_terminal_kernel")


@pytest.fixture(scope="module")
def rig():
    """(the engine, real share_obs rows [5, 40, 29] of a rollout on it, Gaussian rows of the same shape)"""
    import torch
    eng = small_engine(40, False)
    eng.reset()
    g = torch.Generator().manual_seed(12)
    acts = torch.randint(0, 3, (5, 40, 3), dtype=torch.int32, generator=g).cuda()
    real = eng.rollout(acts)[1].clone()
    gauss = torch.randn((5, 40, 29), generator=g).cuda()
    assert real.shape == (5, 40, 29) and bool(real.isfinite().all()) and float(real.std()) > 0.05
    yield eng, real, gauss
    eng.close()


def _bits(x):
    import torch
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("value_norm", [None, CR.VALUE_NORM], ids=["raw", "valuenorm"])
@pytest.mark.parametrize("feature_norm", [True, False], ids=["ln0", "no_ln0"])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_values_match_the_restatement(rig, activation, feature_norm, value_norm):
    import torch
    eng, real, gauss = rig
    sd = CR.make_critic(40 + 2 * feature_norm + (activation == "relu"), feature_norm)
    eng.set_critic(sd, value_norm, activation)
    scale = 1.0 if value_norm is None else float(np.sqrt(value_norm[1]))
    worst = own = 0.0
    for what, rows in (("real", real), ("gaussian", gauss)):
        ref = CR.forward(sd, rows, activation, value_norm)                                       # [5, 40] fp64, once per kind of rows
        own = max(own, float((CR.forward(sd, rows, activation, value_norm, dtype=torch.float32).double() - ref).abs().max()))
        flat = rows.reshape(-1, 29)
        for R in ROW_COUNTS + (tuple(rows.shape),):
            x = rows if isinstance(R, tuple) else flat[:R].contiguous()
            got = eng.critic_values(x)
            assert got.shape == x.shape[:-1] and got.dtype == torch.float32 and eng.last_step_kernel() == "sdc_critic_values_kernel"
            want = ref if isinstance(R, tuple) else ref.reshape(-1)[:R]
            err = float((got.cpu().double() - want).abs().max())
            worst = max(worst, err)
            assert err <= BOUND * scale, (what, R, err)
    print("critic values (%s, feature LayerNorm %s, scale %g): max |error| %.2e, torch fp32 against fp64 on the same rows %.2e"
          % (activation, feature_norm, scale, worst, own))


@pytest.mark.parametrize("dead", [1, 2])
def test_dead_relu_layer_gives_finite_values(rig, dead):
    """every activation of layer `dead` is 0 (its biases are -10): the LayerNorm behind it sees variance 0 and leaves its bias"""
    import torch
    eng, real, gauss = rig
    sd = CR.make_critic(60 + dead)
    key = CR.KEYS["b1" if dead == 1 else "b2"]
    sd[key] = torch.full_like(sd[key], -10.0)
    eng.set_critic(sd, None, "relu")
    for rows in (real, gauss):
        x = rows.double().cpu()
        h = CR._layer_norm(x, sd[CR.KEYS["ln0_g"]].double(), sd[CR.KEYS["ln0_b"]].double())
        pre = h @ sd[CR.KEYS["w1"]].double().T + sd[CR.KEYS["b1"]].double()
        if dead == 2:
            h = CR._layer_norm(torch.relu(pre), sd[CR.KEYS["ln1_g"]].double(), sd[CR.KEYS["ln1_b"]].double())
            pre = h @ sd[CR.KEYS["w2"]].double().T + sd[CR.KEYS["b2"]].double()
        assert float(pre.max()) < -1.0      # (the layer IS dead on these rows)
        got = eng.critic_values(rows)
        assert bool(got.isfinite().all())
        err = float((got.cpu().double() - CR.forward(sd, rows, "relu")).abs().max())
        assert err <= BOUND, (dead, err)


def test_a_rows_value_depends_on_that_row_alone(rig):
    import torch
    eng, real, gauss = rig
    eng.set_critic(CR.make_critic(70), CR.VALUE_NORM, "tanh")
    for rows in (real, gauss):
        flat = rows.reshape(-1, 29)
        v = eng.critic_values(flat)                                    # 200 rows: three full workgroups and one with 8 rows
        back = eng.critic_values(flat.flip(0).contiguous())
        assert torch.equal(_bits(back.flip(0)), _bits(v))
        v64, v17 = eng.critic_values(flat[:64].contiguous()), eng.critic_values(flat[:17].contiguous())
        assert torch.equal(_bits(v17), _bits(v64[:17])) and torch.equal(_bits(v64), _bits(v[:64]))
    # more rows than one pass of the largest grid takes (1024 workgroups of 64 rows): the first two workgroups come round again, the
    # second for a part-filled wavefront
    big = torch.randn((1024 * 64 + 70, 29), generator=torch.Generator().manual_seed(13)).cuda()
    vb = eng.critic_values(big)
    tail = big[-134:].contiguous()
    assert torch.equal(_bits(vb[-134:]), _bits(eng.critic_values(tail))) and torch.equal(_bits(vb[:64]), _bits(eng.critic_values(big[:64].contiguous())))
    sd = CR.make_critic(70)
    assert float((vb[-134:].cpu().double() - CR.forward(sd, tail, "tanh", CR.VALUE_NORM)).abs().max()) <= BOUND * 7.5
    # nothing is stored past the last row: through the C ABI into a buffer of R + 64 entries
    for R in (17, 64, 65):
        buf = torch.full((R + 64,), -12345.0, dtype=torch.float32, device=eng.device)
        x = gauss.reshape(-1, 29)[:R].contiguous()
        stream = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
        assert eng.lib.sdc_critic_values(eng._h, C.c_void_p(x.data_ptr()), R, C.c_void_p(buf.data_ptr()), stream) == 0
        assert torch.equal(_bits(buf[:R]), _bits(eng.critic_values(x))) and bool((buf[R:] == -12345.0).all())


# ---- the planners' terminal value ---------------------------------------------------------------------------------------------------
def _factor(K, gamma, weight):
    """(g_{K-1} * gamma) * weight as the library multiplies it: the discount table by repeated multiplication"""
    g = 1.0
    for _ in range(1, K):
        g = g * gamma
    return (g * gamma) * weight


def _terms(twin, cands, K, weight=WEIGHT, gamma=GAMMA):
    """per candidate (a [K, N, 3] action tensor), from the twin's materialised rollout: factor * (done ? 0 : (double) V) [N] in fp64,
    V = critic_values of the last step's share_obs rows; the twin is where it was afterwards"""
    import torch
    mk = twin.mark(max_steps=K)
    out = []
    for cand in cands:
        o = twin.rollout(cand)
        v = twin.critic_values(o[1][-1].contiguous()).double()
        out.append(torch.where(o[3][-1] != 0, torch.zeros_like(v), v) * _factor(K, gamma, weight))
        twin.rewind(mk)
    return out


def _assert_identity(score_w, score_0, term, what):
    bound = 1e-12 * (score_0.abs() + term.abs())
    err = (score_w - score_0 - term).abs()
    assert bool((err <= bound).all()), (what, float(err.max()))


@pytest.mark.parametrize("mapping", ["default", "quad", "two_steps"])
def test_plan_adds_the_discounted_value_of_the_last_state(mapping):
    import torch
    N, M, K = 40, 3, 4
    flags = {"default": 0, "quad": L.DEBUG_QUAD, "two_steps": L.PLAN_DEBUG_TWO_STEPS}[mapping]
    (a, b, c), g = _twins(N, n=3, debug_flags=flags)
    cand = _cands(M, K, N, g)
    sd = CR.make_critic(80)
    for e in (a, b, c):
        e.set_critic(sd, CR.VALUE_NORM, "tanh")
    a.set_plan_critic(WEIGHT)
    assert a.plan_critic == WEIGHT and b.plan_critic == 0.0
    ra, rb = a.plan(cand, **OBJ), b.plan(cand, **OBJ)
    assert a.last_step_kernel() == "sdc_critic_terminal_kernel" and b.last_step_kernel() not in CRITIC_KERNELS
    if mapping == "quad":
        assert "quad" in b.last_step_kernel()
    terms = _terms(c, [cand[m] for m in range(M)], K)
    for m in range(M):
        assert float(terms[m].abs().min()) > 0.0      # (no episode ends here: every env has a term)
        _assert_identity(ra.score[m], rb.score[m], terms[m], (mapping, m))
    assert torch.equal(ra.returns.view(torch.int64), rb.returns.view(torch.int64))
    assert not torch.equal(ra.score, rb.score)
    best = np.argmax(ra.score.cpu().numpy(), axis=0)      # (NumPy: the first maximum)
    assert np.array_equal(ra.best.cpu().numpy(), best)
    assert torch.equal(ra.action, cand[ra.best.long(), 0, torch.arange(N, device=a.device)])
    for e in (a, b, c):
        e.close()


def test_the_term_is_zero_where_the_horizon_ends_the_episode():
    import torch
    N, M, K, EP = 40, 3, 4, 24
    engs = [_mk(N, ep=EP, auto_reset=False, seed=21) for _ in range(2)]
    g = torch.Generator(device="cpu").manual_seed(4)
    for _ in range(EP - K):
        x = torch.randint(0, 3, (N, 3), dtype=torch.int32, generator=g).cuda()
        for e in engs:
            e.step(x)
    a, b = engs
    assert a.steps_to_episode_end() == K
    cand = _cands(M, K, N, g)
    a.set_critic(CR.make_critic(81), CR.VALUE_NORM, "tanh")
    a.set_plan_critic(WEIGHT)
    ra, rb = a.plan(cand, **OBJ), b.plan(cand, **OBJ)
    assert a.last_step_kernel() == "sdc_critic_terminal_kernel"
    for nm in ("score", "returns", "best", "action"):
        assert torch.equal(getattr(ra, nm).view(torch.uint8), getattr(rb, nm).view(torch.uint8)), nm
    # one step earlier the same engines do see the term
    short = a.plan(cand[:, :K - 1].contiguous(), **OBJ)
    assert not torch.equal(short.score, b.plan(cand[:, :K - 1].contiguous(), **OBJ).score)
    for e in engs:
        e.close()


def test_plan_cem_scores_with_the_value():
    import torch
    N, M, K = 40, 3, 4
    (a, b, c), _ = _twins(N, n=3)
    sd = CR.make_critic(82)
    for e in (a, b, c):
        e.set_critic(sd, None, "relu")
    for e in (a, c):
        e.set_plan_critic(WEIGHT)
    kw = dict(seed=7, draw=1, **OBJ)
    ra, rb = a.plan_cem(K, 1, M, 2, **kw), b.plan_cem(K, 1, M, 2, **kw)
    assert torch.equal(ra.cand, rb.cand)                       # (one seed, one iteration: the same candidates)
    b.set_plan_critic(0.0)
    terms = _terms(b, [ra.cand[m] for m in range(M)], K)
    for m in range(M):
        _assert_identity(ra.cand_score[m], rb.cand_score[m], terms[m], m)
    assert not torch.equal(ra.cand_score, rb.cand_score)
    # two iterations: the candidates and scores the call returns are `plan`'s of those candidates, critic and weight the same
    r2 = a.plan_cem(K, 2, M, 2, **kw)
    assert torch.equal(r2.cand_score.view(torch.int64), c.plan(r2.cand, **OBJ).score.view(torch.int64))
    for e in (a, b, c):
        e.close()


def test_plan_cem_groups_scores_with_the_value():
    import torch
    R, G, K = 4, 10, 4
    N = R * G
    (a, b, c), _ = _twins(N, n=3)
    sd = CR.make_critic(83)
    for e in (a, b, c):
        e.sync_groups(R)
        e.set_critic(sd, CR.VALUE_NORM, "tanh")
    for e in (a, c):
        e.set_plan_critic(WEIGHT)
    kw = dict(seed=9, draw=2, group_base=0, **OBJ)
    ra, rb = a.plan_cem_groups(R, K, 1, 2, **kw), b.plan_cem_groups(R, K, 1, 2, **kw)
    assert torch.equal(ra.cand, rb.cand)
    (term,) = _terms(b, [ra.cand], K)                          # (replicas are env rows: one rollout of the batch)
    _assert_identity(ra.cand_score, rb.cand_score, term, "groups")
    assert not torch.equal(ra.cand_score, rb.cand_score)
    r2 = a.plan_cem_groups(R, K, 2, 2, **kw)
    assert torch.equal(r2.cand_score.view(torch.int64), c.plan(r2.cand[None].contiguous(), **OBJ).score[0].view(torch.int64))
    for e in (a, b, c):
        e.close()


def test_weight_zero_after_a_weight_is_a_plan_that_never_saw_a_critic():
    import torch
    N, M, K = 40, 3, 4
    (a, b), g = _twins(N)
    cand = _cands(M, K, N, g)
    a.set_critic(CR.make_critic(84), CR.VALUE_NORM, "tanh")
    a.set_plan_critic(WEIGHT)
    with_term = a.plan(cand, **OBJ)
    a.set_plan_critic(0.0)
    assert a.plan_critic == 0.0
    kw = dict(seed=3, draw=5, **OBJ)
    for call in (lambda e: e.plan(cand, **OBJ), lambda e: e.plan_cem(K, 2, 4, 2, **kw)):
        ra, rb = call(a), call(b)
        assert a.last_step_kernel() not in CRITIC_KERNELS and a.last_step_kernel() == b.last_step_kernel()
        for nm in ("score", "returns", "best", "action", "cand", "cand_score", "best_score", "probs", "best_seq"):
            if hasattr(ra, nm):
                assert torch.equal(getattr(ra, nm).view(torch.uint8), getattr(rb, nm).view(torch.uint8)), nm
    assert not torch.equal(with_term.score, a.plan(cand, **OBJ).score)
    a.close()
    b.close()


def test_rollout_actor_appends_the_values():
    import torch
    from tests.actor_ref import set_actors, torch_actor
    eng = small_engine(40, False)
    set_actors(eng, [torch_actor(500 + i) for i in range(3)])
    eng.set_critic(CR.make_critic(85), CR.VALUE_NORM, "tanh")
    eng.reset()
    plain = eng.rollout_actor(6)
    assert len(plain) == 7
    out = eng.rollout_actor(6, want_logits=True, want_values=True)
    assert len(out) == 8 and out[7].shape == (6, 40) and out[7].dtype == torch.float32
    assert torch.equal(_bits(out[7]), _bits(eng.critic_values(out[1])))
    eng.close()


def test_deepcopy_of_a_vec_env_carries_the_critic_and_the_weight():
    import torch
    N, M, K = 16, 3, 4
    args = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True}
    a = SustainDCVecEnv(args, n_envs=N, seed=3, months=[6] * N, return_torch=True)
    a.set_critic(CR.make_critic(86), CR.VALUE_NORM, "relu")      # (host and device state of the engine: before reset() as well)
    a.set_plan_critic(WEIGHT)
    a.reset()
    rng = np.random.default_rng(2)
    for _ in range(5):
        a.step(torch.as_tensor(rng.integers(0, 3, (N, 3)).astype(np.int32), device=a.engine.device))
    cand = torch.as_tensor(rng.integers(0, 3, (M, K, N, 3)).astype(np.int32), device=a.engine.device)
    cp = copy.deepcopy(a)
    assert cp.plan_critic == WEIGHT == a.plan_critic
    ra, rc = a.plan(cand, **OBJ), cp.plan(cand, **OBJ)
    for nm in ("score", "returns", "best", "action"):
        assert torch.equal(getattr(ra, nm).view(torch.uint8), getattr(rc, nm).view(torch.uint8)), nm
    x = torch.randn((7, 29), device=a.engine.device)
    assert torch.equal(_bits(a.critic_values(x)), _bits(cp.critic_values(x)))
    a.set_plan_critic(0.0)
    assert cp.plan_critic == WEIGHT                               # (the copy's weight is its own)
    assert not torch.equal(a.plan(cand, **OBJ).score, rc.score)
    a.close()
    cp.close()


def test_refusals():
    import torch
    N = 8
    (a,), g = _twins(N, n=1, history=6)
    x = torch.randn((N, 29), device=a.device)
    vals = torch.empty((N,), dtype=torch.float32, device=a.device)
    stream = C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    # before set_critic
    refused(a, "sdc_set_critic first", lambda: a.critic_values(x))
    refused(a, "no critic is set", lambda: a.set_plan_critic(0.5))
    a.set_plan_critic(0.0)                                        # (0 is always taken)
    assert a.lib.sdc_critic_values(a._h, p(x), N, p(vals), stream) == -2 and b"sdc_set_critic first" in a.lib.sdc_last_error()
    assert a.lib.sdc_set_plan_critic(a._h, 0.5) == -2 and b"no critic is set" in a.lib.sdc_last_error()
    # set_critic's own: the critic in force stays
    sd = CR.make_critic(87)
    a.set_critic(sd, CR.VALUE_NORM, "tanh")
    before = a.critic_values(x).clone()
    bad = dict(sd)
    bad[CR.KEYS["w2"]] = sd[CR.KEYS["w2"]].clone()
    bad[CR.KEYS["w2"]][5, 7] = float("nan")
    refused(a, "not finite", lambda: a.set_critic(bad))
    refused(a, "scale must be positive", lambda: a.set_critic(sd, (0.0, 0.0)))
    refused(a, "scale must be positive", lambda: a.set_critic(dict({k: sd[v] for k, v in CR.KEYS.items()}, scale=-1.0)))
    refused(a, "activation code", lambda: a.set_critic(dict({k: sd[v] for k, v in CR.KEYS.items()}, flags=5)))
    assert a.lib.sdc_set_critic(a._h, None) == -2 and b"null handle or params" in a.lib.sdc_last_error()
    assert torch.equal(_bits(a.critic_values(x)), _bits(before))
    # critic_values: the tensor
    refused(a, r"shape \(\.\.\., 29\)", lambda: a.critic_values(torch.randn((N, 26), device=a.device)))
    refused(a, "CUDA tensor", lambda: a.critic_values(x.cpu()))
    refused(a, "float32", lambda: a.critic_values(x.double()))
    refused(a, "contiguous", lambda: a.critic_values(torch.randn((N, 58), device=a.device)[:, ::2]))
    refused(a, "n_rows = 0", lambda: a.critic_values(x[:0]))
    for args, match in (((None, N, p(vals)), b"null array"), ((p(x), N, None), b"null array"), ((p(x), 0, p(vals)), b"n_rows = 0"),
                        ((p(x), -3, p(vals)), b"n_rows = -3"), ((C.c_void_p(x.data_ptr() + 2), N - 1, p(vals)), b"dword-aligned"),
                        ((p(x), N, C.c_void_p(vals.data_ptr() + 1)), b"dword-aligned")):
        assert a.lib.sdc_critic_values(a._h, *args, stream) == -2 and match in a.lib.sdc_last_error(), match
    # the weight
    a.set_plan_critic(0.25)
    for w in (float("nan"), float("inf"), float("-inf")):
        refused(a, "not finite", lambda: a.set_plan_critic(w))
    assert a.plan_critic == 0.25
    assert a.lib.sdc_get_plan_critic(a._h, None) == -2 and b"null handle or out" in a.lib.sdc_last_error()
    a.close()
    # the concatenated shared-observation layout has no 29-entry rows to value
    args = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": False}
    env = SustainDCVecEnv(args, n_envs=4, seed=1, months=[6] * 4, return_torch=True)
    assert env.share_concat
    with pytest.raises(NotImplementedError, match="concatenated"):
        env.set_critic(sd)
    env.close()
