"""Planning with the cross-entropy method on the device (SdcEngine.plan_cem / SustainDCVecEnv.plan_cem / CEMMPCAgent over sdc_plan_cem)
held to the call's stated arithmetic (include/sustaindc_hip.h): the sampler restated in NumPy on tests/reset_ref.philox4x32_10, the
scores against `plan` on a twin engine, the ranking, the incumbent and the refit restated in torch fp64 -- every comparison bit for bit.

 1. the sampler;  2. the scores;  3. the refit;  4. ties;  5. one call of I iterations against I calls of one;  6. the incumbent's
    score never falls and somewhere rises;  7. the engine afterwards, at 70 and 4 096 envs;  8. the chunked output block;  9. the
    draws are keyed on the global env index;  10. the refusals, each of which leaves the engine untouched;  11. the vector env with
    an agent subset under two CEMMPCAgents.

NOT in verify mode, for the reason tests/test_gpu_plan.py gives (sdc_rollout refuses it; test 10 checks that refusal).  Episodes of 96
steps, rings of 128 keys, as there.  N = 70 unless stated: two workgroups of either kernel, the last one partial, and the general step
kernel.  M = 5 candidates, E = 2 elites, K = 3 steps, I = 3 iterations unless stated."""
import ctypes as C

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import CEMMPCAgent, CEMResult, SustainDCVecEnv
from tests.plan_util import EP, OBJ, _outputs, _twins, objective, planner_refusals, refusal_engines, refused
from tests.plan_util import refit_ref as _refit_ref
from tests.plan_util import sample_ref as _sample_ref
from tests.test_gpu_clone import _acts
from tests.test_gpu_mark import _assert_rewound, _grab, _mk, _same_out

pytestmark = pytest.mark.gpu

N, M, E, K, I = 70, 5, 2, 3, 3
FIELDS = ("action", "best_seq", "best_score", "probs", "cand", "cand_score")


def _probs(K_, N_, seed=3):
    """non-uniform distributions [K, N, 3, 3] with the degenerate rows (0, 0, 1), (1, 0, 0), (0, 1, 0) and (0.25, 0.5, 0.25) in both
    workgroups' envs"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.rand((K_, N_, 3, 3), dtype=torch.float64, generator=g) + 0.05
    p = p / p.sum(-1, keepdim=True)
    rows = [(0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.25, 0.5, 0.25)]
    for i, r in enumerate(rows):
        for n in (i, N_ - 1 - i):
            p[i % K_, n, i % 3] = torch.tensor(r, dtype=torch.float64)
            p[(i + 1) % K_, n, (i + 1) % 3] = torch.tensor(r, dtype=torch.float64)
    return p.cuda()


def _seq(K_, N_, seed=4):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 3, (K_, N_, 3), dtype=torch.int32, generator=g).cuda()


def _same(ra, rb, what, fields=FIELDS):
    import torch
    for nm in fields:
        u, v = getattr(ra, nm), getattr(rb, nm)
        assert u.dtype == v.dtype and torch.equal(u, v), (what, nm, (u != v).nonzero()[:4].tolist())


def test_sampling_bit_for_bit():
    import torch
    (b,), _ = _twins(N, n=1)
    p0, s0 = _probs(K, N), _seq(K, N)
    kw = dict(seed=0x1234567_89ABCDEF, draw=7, iter0=5)
    res = b.plan_cem(K, 1, M, E, probs=p0.clone(), best_seq=s0.clone(), **kw)
    assert isinstance(res, CEMResult)
    assert res.cand.shape == (M, K, N, 3) and res.cand.dtype == torch.int32 and res.cand_score.shape == (M, N)
    assert res.best_score.shape == (1, N) and res.action.shape == (N, 3) and res.probs.shape == (K, N, 3, 3)
    assert torch.equal(res.cand[0], s0), "candidate 0 is the incumbent passed in"
    ref = _sample_ref(p0, M, kw["seed"], 7, 5)
    got = res.cand[1:].cpu().numpy()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:6].tolist()
    assert len(np.unique(got)) == 3 and not np.array_equal(got[0], got[1])
    # the degenerate rows draw what they must
    pc = p0.cpu()
    sure = (pc == 1.0).nonzero()
    assert len(sure) >= 12
    for k_, n_, a_, j_ in sure.tolist():
        assert (got[:, k_, n_, a_] == j_).all(), (k_, n_, a_, j_)
    # the same arguments reproduce the candidates; another draw, seed or iteration index changes them
    again = b.plan_cem(K, 1, M, E, probs=p0.clone(), best_seq=s0.clone(), **kw)
    _same(res, again, "the same arguments")
    for other in (dict(draw=8), dict(seed=kw["seed"] ^ (1 << 40)), dict(seed=kw["seed"] ^ 1), dict(iter0=6)):
        o = dict(kw, **other)
        r2 = b.plan_cem(K, 1, M, E, probs=p0.clone(), best_seq=s0.clone(), **o)
        assert not torch.equal(r2.cand[1:], res.cand[1:]), other
        assert np.array_equal(r2.cand[1:].cpu().numpy(), _sample_ref(p0, M, o["seed"], o["draw"], o["iter0"])), other
        assert torch.equal(r2.cand[0], s0)
    # a fixed column is constant in the sampled candidates, the others are drawn as before; the incumbent keeps its own
    fx = b.plan_cem(K, 1, M, E, probs=p0.clone(), best_seq=s0.clone(), fixed_action=(-1, 2, -1), **kw)
    assert bool((fx.cand[1:, ..., 1] == 2).all()) and torch.equal(fx.cand[0], s0)
    assert np.array_equal(fx.cand[1:].cpu().numpy(), _sample_ref(p0, M, kw["seed"], 7, 5, fixed=(-1, 2, -1)))
    assert torch.equal(fx.probs[:, :, 1], p0[:, :, 1]) and not torch.equal(fx.probs[:, :, 0], p0[:, :, 0])
    # the defaults: uniform distributions, the do-nothing incumbent
    d = b.plan_cem(K, 1, M, E, **kw)
    third = torch.full((K, N, 3, 3), 1.0 / 3.0, dtype=torch.float64, device=b.device)
    assert np.array_equal(d.cand[1:].cpu().numpy(), _sample_ref(third, M, kw["seed"], 7, 5))
    assert torch.equal(d.cand[0], torch.tensor([1, 1, 2], dtype=torch.int32, device=b.device).expand(K, N, 3))
    b.close()


def test_scores_equal_plan_on_a_twin_engine():
    import torch
    (b, twin), _ = _twins(N)
    res = b.plan_cem(K, 1, M, E, probs=_probs(K, N), best_seq=_seq(K, N), seed=11, **OBJ)
    ref = twin.plan(res.cand, **OBJ)
    assert torch.equal(res.cand_score, ref.score), (res.cand_score - ref.score).abs().max().item()
    assert not torch.equal(ref.score[0], ref.score[1])
    assert not torch.equal(twin.plan(res.cand).score, ref.score)      # (the objective matters)
    b.close()
    twin.close()


@pytest.mark.parametrize("alpha,p_min", [(0.3, 0.02), (0.0, 0.0)])
def test_refit_bit_for_bit(alpha, p_min):
    import torch
    (b,), _ = _twins(N, n=1)
    p0, s0 = _probs(K, N), _seq(K, N)
    res = b.plan_cem(K, 1, M, E, probs=p0.clone(), best_seq=s0.clone(), seed=5, alpha=alpha, p_min=p_min, **OBJ)
    elite, best, seq, top, p = _refit_ref(res.cand, res.cand_score, p0, s0, E, alpha, p_min)
    assert bool((elite.sum(0) == E).all()) and len(torch.unique(best)) > 1
    assert torch.equal(res.best_seq, seq)
    assert torch.equal(res.best_score[0], top)
    assert torch.equal(res.action, seq[0])
    assert torch.equal(res.probs, p), ((res.probs - p).abs().max().item(), (res.probs != p).nonzero()[:4].tolist())
    assert bool(((res.probs.sum(-1) - 1.0).abs() < 1e-15).all())
    if p_min > 0.0:
        assert bool((res.probs >= p_min / (1.0 + 3 * p_min) * (1.0 - 1e-12)).all())      # (q >= p_min, s <= 1 + 3 p_min)
    else:      # the elites' frequencies, to the bit: multiples of 1 / E
        assert bool(((res.probs * E).round() == res.probs * E).all())
    # a fixed agent keeps its distributions and counts for nothing in the others'
    fx = b.plan_cem(K, 1, M, E, probs=p0.clone(), best_seq=s0.clone(), seed=5, alpha=alpha, p_min=p_min, fixed_action=(1, -1, -1), **OBJ)
    _, _, seq2, top2, p2 = _refit_ref(fx.cand, fx.cand_score, p0, s0, E, alpha, p_min, fixed=(1, -1, -1))
    assert torch.equal(fx.probs, p2) and torch.equal(fx.probs[:, :, 0], p0[:, :, 0])
    assert torch.equal(fx.best_seq, seq2) and torch.equal(fx.best_score[0], top2)
    # three elites of six candidates, four steps: another E, odd counts
    r3 = b.plan_cem(4, 1, 6, 3, probs=_probs(4, N), best_seq=_seq(4, N), seed=6, alpha=alpha, p_min=p_min, **OBJ)
    _, _, seq3, top3, p3 = _refit_ref(r3.cand, r3.cand_score, _probs(4, N), _seq(4, N), 3, alpha, p_min)
    assert torch.equal(r3.probs, p3) and torch.equal(r3.best_seq, seq3) and torch.equal(r3.best_score[0], top3)
    b.close()


def test_ties_go_to_the_lower_candidate():
    import torch
    (b,), _ = _twins(N, n=1)
    p0, s0 = _probs(K, N), _seq(K, N)
    res = b.plan_cem(K, 2, M, E, probs=p0.clone(), best_seq=s0.clone(), seed=5, reward_weights=(0.0, 0.0, 0.0))
    assert not bool(res.cand_score.any()) and not bool(res.best_score.any())
    assert torch.equal(res.best_seq, s0) and torch.equal(res.action, s0[0])
    # the elites are candidates 0 .. E-1: the distributions are their frequencies (alpha = 0, p_min = 0)
    first = b.plan_cem(K, 1, M, E, probs=p0.clone(), best_seq=s0.clone(), seed=5, reward_weights=(0.0, 0.0, 0.0))
    hit = first.cand[:E, ..., None] == torch.arange(3, device=b.device, dtype=torch.int32)
    assert torch.equal(first.probs, hit.sum(0).double() / float(E))
    elite, best, _, _, p = _refit_ref(first.cand, first.cand_score, p0, s0, E, 0.0, 0.0)
    assert bool(elite[:E].all()) and not bool(elite[E:].any()) and not bool(best.any()) and torch.equal(first.probs, p)
    b.close()


def test_one_call_of_three_iterations_equals_three_calls_of_one():
    import torch
    (a, b), _ = _twins(N)
    p0, s0 = _probs(K, N), _seq(K, N)
    kw = dict(seed=77, draw=3, alpha=0.3, p_min=0.02, **OBJ)
    whole = a.plan_cem(K, I, M, E, probs=p0.clone(), best_seq=s0.clone(), iter0=0, **kw)
    probs, seq, rows, cands = p0.clone(), s0.clone(), [], []
    for it in range(I):
        before = probs.clone()
        r = b.plan_cem(K, 1, M, E, probs=probs, best_seq=seq, iter0=it, **kw)
        assert r.probs is probs and r.best_seq is seq      # (updated in place and returned)
        # (the iteration's index is in the generator's counter: without it the two sides would still agree with each other)
        assert np.array_equal(r.cand[1:].cpu().numpy(), _sample_ref(before, M, 77, 3, it)), it
        rows.append(r.best_score[0].clone())
        cands.append(r.cand.clone())
    assert torch.equal(whole.best_score, torch.stack(rows))
    _same(whole, r, "the last of three calls", fields=("action", "best_seq", "probs", "cand", "cand_score"))
    assert not torch.equal(cands[0][1:], cands[1][1:]) and not torch.equal(cands[1][1:], cands[2][1:])
    assert not torch.equal(whole.probs, p0)
    a.close()
    b.close()


def test_incumbent_score_never_falls_and_beats_do_nothing_somewhere():
    import torch
    (b, twin), _ = _twins(N)
    res = b.plan_cem(K, I, M, E, seed=1, alpha=0.3, p_min=0.02, **OBJ)
    nothing = torch.tensor([1, 1, 2], dtype=torch.int32, device=b.device).expand(1, K, N, 3).contiguous()
    base = twin.plan(nothing, **OBJ).score[0]
    s = res.best_score
    print("envs above do-nothing after each iteration:", [(s[i] > base).sum().item() for i in range(I)])
    assert bool((s[0] >= base).all())
    for i in range(I - 1):
        assert bool((s[i + 1] >= s[i]).all()), i
    assert bool((s[0] > base).any()) and bool((s[I - 1] > s[0]).any())
    # the sequence returned scores what the call says it does
    assert torch.equal(twin.plan(res.best_seq[None].contiguous(), **OBJ).score[0], s[I - 1])
    assert torch.equal(res.action, res.best_seq[0])
    b.close()
    twin.close()


@pytest.mark.parametrize("n_envs", [N, 4096])
def test_the_engine_afterwards(n_envs):
    import torch
    (a, b), g = _twins(n_envs)
    kernel = b.last_step_kernel()
    kept, before = _outputs(b), _grab(b)
    left = b.steps_to_episode_end()
    res = b.plan_cem(K, I, M, E, seed=2, alpha=0.3, p_min=0.02, **OBJ)
    assert res.best_score.shape == (I, n_envs)
    _assert_rewound(b, before, "after plan_cem")
    assert b.steps_to_episode_end() == left
    for nm, x in kept.items():
        assert torch.equal(getattr(b, nm).view(torch.uint8), x.view(torch.uint8)), nm
    x = _acts(n_envs, g)
    a.step(x)
    b.step(x)
    _same_out(a, b, "the step after")
    assert b.last_step_kernel() == kernel == a.last_step_kernel()
    if n_envs == 4096:
        assert kernel == "sdc_dynamics_fast_kernel"
    # the call used up the envs' one live mark
    mk = b.mark(max_steps=4)
    b.plan_cem(2, 1, 2, 1)
    with pytest.raises(ValueError, match="dead"):
        b.rewind(mk)
    a.close()
    b.close()


def test_chunked_output_block_gives_the_unchunked_results():
    whole = _twins(N, n=1)[0][0]
    chunked = _twins(N, n=1, debug_flags=L.PLAN_DEBUG_TWO_STEPS)[0][0]      # (chunks of 2 + 1 steps)
    kw = dict(probs=None, best_seq=None, seed=9, alpha=0.3, p_min=0.02, **OBJ)
    _same(whole.plan_cem(K, I, M, E, **kw), chunked.plan_cem(K, I, M, E, **kw), "chunked against whole")
    whole.close()
    chunked.close()


def test_draws_are_keyed_on_the_global_env_index():
    import torch
    LO = 32
    big, part = _mk(N, ep=EP, seed=21), _mk(N - LO, ep=EP, seed=21, env_index_base=LO)
    g = torch.Generator(device="cpu").manual_seed(21)
    for _ in range(20):
        x = _acts(N, g)
        big.step(x)
        part.step(x[LO:].contiguous())
    p0, s0 = _probs(K, N), _seq(K, N)
    kw = dict(seed=13, draw=2, alpha=0.3, p_min=0.02, **OBJ)
    ra = big.plan_cem(K, I, M, E, probs=p0.clone(), best_seq=s0.clone(), **kw)
    rb = part.plan_cem(K, I, M, E, probs=p0[:, LO:].contiguous(), best_seq=s0[:, LO:].contiguous(), **kw)
    assert torch.equal(ra.cand[:, :, LO:], rb.cand)
    assert torch.equal(ra.cand_score[:, LO:], rb.cand_score)
    assert torch.equal(ra.probs[:, LO:], rb.probs)
    assert torch.equal(ra.best_seq[:, LO:], rb.best_seq) and torch.equal(ra.best_score[:, LO:], rb.best_score)
    big.close()
    part.close()


def test_refusals_leave_the_engine_untouched():
    import torch
    n = 8
    a, fresh, verify, late = refusal_engines(n)

    # what sdc_plan refuses
    planner_refusals(lambda e, K, **kw: e.plan_cem(K, 1, 2, 1, **kw), "n_steps", a, fresh, verify, late)
    refused(a, "n_steps", lambda: a.plan_cem(0, 1, 2, 1))
    # the parameters' ranges
    refused(a, "n_iters", lambda: a.plan_cem(3, 0, 2, 1))
    refused(a, "iter0", lambda: a.plan_cem(3, 1, 2, 1, iter0=-1))
    refused(a, "iter0", lambda: a.plan_cem(3, 2, 2, 1, iter0=65535))
    refused(a, "n_cand", lambda: a.plan_cem(3, 1, 1, 1))
    refused(a, "n_cand", lambda: a.plan_cem(3, 1, L.CEM_MAX_CAND + 1, 1))
    refused(a, "n_elite", lambda: a.plan_cem(3, 1, 4, 0))
    refused(a, "n_elite", lambda: a.plan_cem(3, 1, 4, 5))
    refused(a, "fixed_action", lambda: a.plan_cem(3, 1, 4, 2, fixed_action=(-1, 3, -1)))
    refused(a, "fixed_action", lambda: a.plan_cem(3, 1, 4, 2, fixed_action=(-2, 0, 0)))
    refused(a, "three integers", lambda: a.plan_cem(3, 1, 4, 2, fixed_action=(-1, -1)))
    for bad in (1.0, -0.1, float("nan")):
        refused(a, "alpha", lambda: a.plan_cem(3, 1, 4, 2, alpha=bad))
    for bad in (0.34, -0.01, float("nan")):
        refused(a, "p_min", lambda: a.plan_cem(3, 1, 4, 2, p_min=bad))
    # malformed tensors
    third = torch.full((3, n, 3, 3), 1.0 / 3.0, dtype=torch.float64, device=a.device)
    seq = torch.ones((3, n, 3), dtype=torch.int32, device=a.device)
    refused(a, "probs must be", lambda: a.plan_cem(3, 1, 4, 2, probs=third.float()))
    refused(a, "probs must be", lambda: a.plan_cem(3, 1, 4, 2, probs=third[:2]))
    refused(a, "probs must be", lambda: a.plan_cem(3, 1, 4, 2, probs=third.cpu()))
    refused(a, "best_seq must be", lambda: a.plan_cem(3, 1, 4, 2, best_seq=seq.long()))
    refused(a, "best_seq must be", lambda: a.plan_cem(3, 1, 4, 2, best_seq=torch.ones((3, n + 1, 3), dtype=torch.int32, device=a.device)))
    refused(a, "best_seq must be", lambda: a.plan_cem(3, 1, 4, 2, best_seq=torch.ones((6, n, 3), dtype=torch.int32, device=a.device)[::2]))
    # what the Python surface cannot send: straight to the library
    arrays = [third.clone(), seq.clone(), torch.empty((1, n), dtype=torch.float64, device=a.device),
              torch.empty((n, 3), dtype=torch.int32, device=a.device), torch.empty((4, 3, n, 3), dtype=torch.int32, device=a.device),
              torch.empty((4, n), dtype=torch.float64, device=a.device)]
    p = lambda t: C.c_void_p(t.data_ptr())

    def params():
        c = L.SdcCemParams()
        c.n_iters, c.iter0, c.n_cand, c.n_elite, c.draw, c.seed, c.alpha, c.p_min = 1, 0, 4, 2, 0, 0, 0.0, 0.0
        c.fixed_action[:] = [-1, -1, -1]
        return c

    def raw(null=None, cem=params(), obj=None, no_cem=False):
        ptrs = [None if i == null else p(t) for i, t in enumerate(arrays)]
        rc = a.lib.sdc_plan_cem(a._h, 3, None if no_cem else C.byref(cem), C.byref(obj) if obj is not None else None, *ptrs, p(a.obs),
                                p(a.share_obs), a._stream())
        a._refused(rc)

    for i in range(len(arrays)):
        refused(a, "null array", lambda: raw(null=i))
    refused(a, "null cem", lambda: raw(no_cem=True))
    refused(a, "n_cols", lambda: raw(obj=objective(L.PLAN_MAX_COLS + 1, 0)))
    refused(a, "n_cols", lambda: raw(obj=objective(-1, 0)))
    refused(a, "info column", lambda: raw(obj=objective(1, L.INFO_DIM)))
    refused(a, "info column", lambda: raw(obj=objective(1, -1)))
    # ... and the calls next to them go through: a NULL objective is the default one; the bounds themselves
    raw()
    torch.cuda.synchronize()
    ok = a.plan_cem(3, 1, 4, 2, probs=third.clone(), best_seq=seq.clone())
    assert torch.equal(arrays[5], ok.cand_score) and torch.equal(arrays[0], ok.probs) and torch.equal(arrays[3], ok.action)
    assert a.plan_cem(37, 1, 2, 2, iter0=65535, alpha=0.999, p_min=1.0 / 3.0).best_score.shape == (1, n) and a.steps_to_episode_end() == 38
    assert late.plan_cem(2, 2, L.CEM_MAX_CAND, 1, fixed_action=(2, 0, -1)).cand.shape == (L.CEM_MAX_CAND, 2, n, 3)
    assert late.steps_to_episode_end() == 2
    for e in (a, fresh, verify, late):
        e.close()


def test_vec_env_plan_cem_with_an_agent_subset_under_two_agents():
    import torch
    n = 16
    args = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True,
            "agents": ["agent_dc", "agent_bat"]}
    a = SustainDCVecEnv(args, n_envs=n, seed=3, months=[6] * n, return_torch=True)
    b = SustainDCVecEnv(args, n_envs=n, seed=3, months=[6] * n, return_torch=True)
    with pytest.raises(ValueError, match="reset"):
        a.plan_cem(3, 1, 4, 2)
    a.reset()
    b.reset()
    kw = dict(n_candidates=6, n_elite=2, n_iters=2, horizon=4, alpha=0.3, p_min=0.02, reward_weights=(0.0, 1.0, 1.0), gamma=0.9,
              info_weights={"bat_CO2_footprint": -1e-3})
    pa, pb, other = CEMMPCAgent(seed=4, **kw), CEMMPCAgent(seed=4, **kw), CEMMPCAgent(seed=5, **kw)
    differs = not torch.equal(other.act(a), CEMMPCAgent(seed=4, **kw).act(a))
    moved = False
    for t in range(10):
        xa, xb = pa.act(a), pb.act(b)
        assert xa.shape == (n, 2) and xa.dtype == torch.int32 and torch.equal(xa, xb), t
        r = pa.last
        assert pa.draw == t + 1 and pa.last_horizon == 4
        assert torch.equal(xa, r.best_seq[0][:, 1:]) and torch.equal(r.best_score, pb.last.best_score)
        assert bool((r.cand[1:, ..., 0] == 1).all())      # the slot outside the subset carries 1 in every sampled candidate
        assert torch.equal(r.probs[:, :, 0], torch.full((4, n, 3), 1.0 / 3.0, dtype=torch.float64, device=r.probs.device))
        assert bool((r.best_score[1] >= r.best_score[0]).all())
        moved = moved or bool((r.best_seq[..., 1:] != torch.tensor([1, 2], dtype=torch.int32, device=r.best_seq.device)).any())
        for u, v in zip(a.step(xa)[:4], b.step(xb)[:4]):
            assert torch.equal(u, v), t
    assert differs and moved
    a.close()
    b.close()
