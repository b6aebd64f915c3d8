"""Planning with the cross-entropy method over replica groups (SdcEngine.plan_cem_groups / sync_groups, SustainDCVecEnv.plan_cem_groups,
GroupCEMMPCAgent over sdc_plan_cem_groups) held to the call's stated arithmetic (include/sustaindc_hip.h): the sampler restated in
NumPy on tests/reset_ref.philox4x32_10, the ranking, the incumbent and the refit restated in torch fp64 (_refit_ref: the header's rules
with "candidate m of env n" read as "replica r of group g"), and the whole call against plan_cem on an engine of G envs -- every
comparison bit for bit.

 1. the sampler;  2. the refit;  3. ties;  4. equals plan_cem;  5. one call of I iterations against I calls of one;  6. the engine
    afterwards;  7. replicas stay in sync over three decisions;  8. the chunked output block;  9. the refusals, each of which leaves
    the engine untouched;  10. GroupCEMMPCAgent across an auto-reset;  11. the vector env with an agent subset.

Shapes (G groups, R replicas, K steps): (3, 2, 1) the smallest group, 32 groups' worth of rows in a wavefront's reach; (5, 13, 4) N = 65:
groups straddle a wavefront, the last wavefront is partial; (2, 65, 3) a group one replica past a wavefront: the refit workgroup's
second wavefront holds one replica; (1, 192, 2) three full wavefronts of replicas, 576 dwords of rows per step; (1, 1024, 2) the largest
group: every thread of the refit workgroup ranks, every LDS array is full.  Episodes of 96 steps, rings of 128 keys, NOT in verify mode,
as tests/test_gpu_cem.py."""
import ctypes as C

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import GroupCEMMPCAgent, GroupCEMResult, SustainDCVecEnv
from tests.plan_util import EP, OBJ, RSV, _outputs, _twins, objective, planner_refusals, refusal_engines, refused, sample_ref
from tests.plan_util import refit_ref as _refit_ref
from tests.test_gpu_clone import _acts
from tests.test_gpu_mark import _assert_rewound, _grab, _mk

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 1), (5, 13, 4), (2, 65, 3), (1, 192, 2), (1, 1024, 2)]
FIELDS = ("action", "step_actions", "best_seq", "best_score", "probs", "cand", "cand_score")


def _gprobs(K_, G_, seed=3):
    """non-uniform distributions [K, G, 3, 3] with the degenerate rows (0, 0, 1), (1, 0, 0), (0, 1, 0) in the first and last group"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.rand((K_, G_, 3, 3), dtype=torch.float64, generator=g) + 0.05
    p = p / p.sum(-1, keepdim=True)
    for i, r in enumerate([(0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]):
        for n in (0, G_ - 1):
            p[i % K_, n, i] = torch.tensor(r, dtype=torch.float64)
    return p.cuda()


def _gseq(K_, G_, seed=4):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 3, (K_, G_, 3), dtype=torch.int32, generator=g).cuda()


def _sample_ref(probs, best_seq, R, seed, draw, it, base=0, fixed=(-1, -1, -1)):
    """cand [K, G R, 3] by the header's rule: replica 0 the incumbent; replica r >= 1 one philox4x32_10 block per (r, k, g), counter
    (r K + k, base + g, draw, (it << 16) | 0xCE3D), key (seed lo, seed hi); u = word * 2^-32; action = (u >= p0) + (u >= p0 + p1)"""
    sampled = sample_ref(probs, R, seed, draw, it, base, fixed)      # replicas 1 .. R-1 [R-1, K, G, 3]
    out = np.concatenate([best_seq.cpu().numpy()[None], sampled]).transpose(1, 2, 0, 3)
    return np.ascontiguousarray(out).reshape(out.shape[0], out.shape[1] * R, 3)


def _as_candidates(res, R):
    """a GroupCEMResult's cand [K, G R, 3] / cand_score [G R] in plan_cem's layout: [R, K, G, 3] / [R, G]"""
    K_, N_ = res.cand.shape[0], res.cand.shape[1]
    return res.cand.view(K_, N_ // R, R, 3).permute(2, 0, 1, 3).contiguous(), res.cand_score.view(N_ // R, R).t().contiguous()


def _same(ra, rb, what, fields=FIELDS):
    import torch
    for nm in fields:
        u, v = getattr(ra, nm), getattr(rb, nm)
        assert u.dtype == v.dtype and torch.equal(u, v), (what, nm, (u != v).nonzero()[:4].tolist())


def _grouped(G, R, history=20, seed=21, **kw):
    """an engine of G R envs after `history` random steps whose groups have then been made copies of their first envs"""
    (e,), g = _twins(G * R, n=1, history=history, seed=seed, **kw)
    e.sync_groups(R)
    return e, g


@pytest.mark.parametrize("G,R,K", SHAPES)
def test_sampling_bit_for_bit(G, R, K):
    import torch
    N = G * R
    b = _mk(N, ep=EP, seed=21)
    p0, s0 = _gprobs(K, G), _gseq(K, G)
    kw = dict(seed=0x1234567_89ABCDEF, draw=7, iter0=5)
    res = b.plan_cem_groups(R, K, 1, 1, probs=p0.clone(), best_seq=s0.clone(), **kw)
    assert isinstance(res, GroupCEMResult)
    assert res.cand.shape == (K, N, 3) and res.cand.dtype == torch.int32 and res.cand_score.shape == (N,)
    assert res.best_score.shape == (1, G) and res.action.shape == (G, 3) and res.step_actions.shape == (N, 3)
    assert res.probs.shape == (K, G, 3, 3) and res.best_seq.shape == (K, G, 3)
    ref = _sample_ref(p0, s0, R, kw["seed"], 7, 5)
    got = res.cand.cpu().numpy()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:6].tolist()
    assert torch.equal(res.cand[:, ::R], s0), "replica 0 is the incumbent passed in"
    if N * K >= 64:
        assert len(np.unique(got)) == 3
    # the degenerate rows draw what they must
    for k_, g_, a_, j_ in (p0.cpu() == 1.0).nonzero().tolist():
        assert (got[k_, g_ * R + 1:(g_ + 1) * R, a_] == j_).all(), (k_, g_, a_, j_)
    # another draw, seed or iteration index changes the samples, each as restated
    for other in (dict(draw=8), dict(seed=kw["seed"] ^ (1 << 40)), dict(seed=kw["seed"] ^ 1), dict(iter0=6)):
        o = dict(kw, **other)
        r2 = b.plan_cem_groups(R, K, 1, 1, probs=p0.clone(), best_seq=s0.clone(), **o)
        assert np.array_equal(r2.cand.cpu().numpy(), _sample_ref(p0, s0, R, o["seed"], o["draw"], o["iter0"])), other
        if N * K >= 64:
            assert not torch.equal(r2.cand, res.cand), other
    # a fixed column is constant in the sampled replicas, the others are drawn as before; the incumbent keeps its own
    fx = b.plan_cem_groups(R, K, 1, 1, probs=p0.clone(), best_seq=s0.clone(), fixed_action=(-1, 2, -1), **kw)
    assert np.array_equal(fx.cand.cpu().numpy(), _sample_ref(p0, s0, R, kw["seed"], 7, 5, fixed=(-1, 2, -1)))
    assert torch.equal(fx.probs[:, :, 1], p0[:, :, 1])
    # the defaults: uniform distributions, the do-nothing incumbent
    d = b.plan_cem_groups(R, K, 1, 1, **kw)
    third = torch.full((K, G, 3, 3), 1.0 / 3.0, dtype=torch.float64, device=b.device)
    nothing = torch.tensor([1, 1, 2], dtype=torch.int32, device=b.device).expand(K, G, 3)
    assert np.array_equal(d.cand.cpu().numpy(), _sample_ref(third, nothing, R, kw["seed"], 7, 5))
    b.close()


def test_draws_are_keyed_on_the_global_group_index():
    import torch
    R, K = 13, 4
    big, part = _mk(4 * R, ep=EP, seed=21), _mk(2 * R, ep=EP, seed=21, env_index_base=2 * R)
    p0, s0 = _gprobs(K, 4), _gseq(K, 4)
    kw = dict(seed=13, draw=2, iter0=1)
    ra = big.plan_cem_groups(R, K, 1, 2, probs=p0.clone(), best_seq=s0.clone(), **kw)
    rb = part.plan_cem_groups(R, K, 1, 2, probs=p0[:, 2:].contiguous(), best_seq=s0[:, 2:].contiguous(), **kw)      # group_base = 2
    rc = part.plan_cem_groups(R, K, 1, 2, probs=p0[:, 2:].contiguous(), best_seq=s0[:, 2:].contiguous(), group_base=2, **kw)
    r0 = part.plan_cem_groups(R, K, 1, 2, probs=p0[:, 2:].contiguous(), best_seq=s0[:, 2:].contiguous(), group_base=0, **kw)
    assert torch.equal(ra.cand[:, 2 * R:], rb.cand) and torch.equal(rb.cand, rc.cand) and not torch.equal(r0.cand, rb.cand)
    assert np.array_equal(rb.cand.cpu().numpy(), _sample_ref(p0[:, 2:], s0[:, 2:], R, 13, 2, 1, base=2))
    odd = _mk(2 * R, ep=EP, seed=21, env_index_base=R + 1)
    with pytest.raises(ValueError, match="does not divide env_index_base"):
        odd.plan_cem_groups(R, K, 1, 2)
    assert odd.plan_cem_groups(R, K, 1, 2, group_base=1).cand.shape == (K, 2 * R, 3)
    for e in (big, part, odd):
        e.close()


@pytest.mark.parametrize("G,R,K", SHAPES)
def test_refit_bit_for_bit(G, R, K):
    import torch
    N, E = G * R, max(1, R // 3)
    b = _mk(N, ep=EP, seed=21)      # (the replicas' states differ: the refit is restated from the scores the call returns)
    g = torch.Generator(device="cpu").manual_seed(2)
    for _ in range(3):
        b.step(_acts(N, g))
    p0, s0 = _gprobs(K, G), _gseq(K, G)
    for alpha, p_min in ((0.3, 0.02), (0.0, 0.0)):
        res = b.plan_cem_groups(R, K, 1, E, probs=p0.clone(), best_seq=s0.clone(), seed=5, alpha=alpha, p_min=p_min, **OBJ)
        cand, score = _as_candidates(res, R)
        elite, best, seq, top, p = _refit_ref(cand, score, p0, s0, E, alpha, p_min)
        assert bool((elite.sum(0) == E).all())
        assert torch.equal(res.best_seq, seq)
        assert torch.equal(res.best_score[0], top)
        assert torch.equal(res.action, seq[0])
        assert torch.equal(res.step_actions, seq[0].repeat_interleave(R, dim=0))
        assert torch.equal(res.probs, p), ((res.probs - p).abs().max().item(), (res.probs != p).nonzero()[:4].tolist())
        assert bool(((res.probs.sum(-1) - 1.0).abs() < 1e-15).all())
        if p_min == 0.0:
            # the elites' frequencies cnt / E: each quotient and the product by E round once (relative 2^-53 each), the sum of the three
            # quotients is within three roundings of 1 and the division by it rounds once more -- p E is within 8 E 2^-53 of a count
            assert bool(((res.probs * E).round() - res.probs * E).abs().max() <= 8 * E * 2.0 ** -53)
        # an unbeaten incumbent's bits stay as they were
        kept = (best == 0).nonzero().flatten()
        assert torch.equal(res.best_seq[:, kept], s0[:, kept])
        # a fixed agent keeps its distributions and counts for nothing in the others'
        fx = b.plan_cem_groups(R, K, 1, E, probs=p0.clone(), best_seq=s0.clone(), seed=5, alpha=alpha, p_min=p_min,
                               fixed_action=(1, -1, -1), **OBJ)
        cand, score = _as_candidates(fx, R)
        _, _, seq2, top2, p2 = _refit_ref(cand, score, p0, s0, E, alpha, p_min, fixed=(1, -1, -1))
        assert torch.equal(fx.probs, p2) and torch.equal(fx.probs[:, :, 0], p0[:, :, 0])
        assert torch.equal(fx.best_seq, seq2) and torch.equal(fx.best_score[0], top2)
    if R >= 13:
        assert len(torch.unique(score)) > 1
    # an incumbent nothing beats: the do-nothing sequence is passed in, E = R, and its bits come back
    keep = b.plan_cem_groups(R, K, 1, R, probs=p0.clone(), best_seq=s0.clone(), seed=5, reward_weights=(0.0, 0.0, 0.0))
    assert torch.equal(keep.best_seq, s0)
    b.close()


def test_ties_go_to_the_lower_replica():
    import torch
    G, R, K, E = 5, 13, 4, 3
    b = _mk(G * R, ep=EP, seed=21)
    p0, s0 = _gprobs(K, G), _gseq(K, G)
    res = b.plan_cem_groups(R, K, 2, E, probs=p0.clone(), best_seq=s0.clone(), seed=5, reward_weights=(0.0, 0.0, 0.0))
    assert not bool(res.cand_score.any()) and not bool(res.best_score.any())
    assert torch.equal(res.best_seq, s0) and torch.equal(res.action, s0[0])
    # the best is replica 0 and the elites are replicas 0 .. E-1: the distributions are their frequencies (alpha = 0, p_min = 0)
    first = b.plan_cem_groups(R, K, 1, E, probs=p0.clone(), best_seq=s0.clone(), seed=5, reward_weights=(0.0, 0.0, 0.0))
    cand, score = _as_candidates(first, R)
    hit = cand[:E, ..., None] == torch.arange(3, device=b.device, dtype=torch.int32)
    assert torch.equal(first.probs, hit.sum(0).double() / float(E))
    elite, best, _, _, p = _refit_ref(cand, score, p0, s0, E, 0.0, 0.0)
    assert bool(elite[:E].all()) and not bool(elite[E:].any()) and not bool(best.any()) and torch.equal(first.probs, p)
    b.close()


@pytest.mark.parametrize("G,R,base", [(3, 8, 0), (2, 64, 5)])
def test_equals_plan_cem_on_an_engine_of_g_envs(G, R, base):
    import torch
    K, I, E = 4, 2, max(1, R // 4)
    (small,), _ = _twins(G, n=1, env_index_base=base)
    big = _mk(G * R, ep=EP, seed=33)
    big.restore(small.snapshot(), envs=np.arange(G * R), rows=np.arange(G * R) // R)      # group g holds the small engine's env g
    assert "reserved" not in OBJ["info_weights"] and len(OBJ["info_weights"]) >= 1
    p0, s0 = _gprobs(K, G), _gseq(K, G)
    kw = dict(seed=99, draw=4, iter0=3, alpha=0.3, p_min=0.02, **OBJ)
    ref = small.plan_cem(K, I, R, E, probs=p0.clone(), best_seq=s0.clone(), **kw)
    res = big.plan_cem_groups(R, K, I, E, probs=p0.clone(), best_seq=s0.clone(), group_base=base, **kw)
    cand, score = _as_candidates(res, R)
    assert torch.equal(score, ref.cand_score), (score - ref.cand_score).abs().max().item()
    assert torch.equal(cand, ref.cand)
    for nm in ("probs", "best_seq", "best_score", "action"):
        u, v = getattr(res, nm), getattr(ref, nm)
        assert u.dtype == v.dtype and torch.equal(u, v), (nm, (u != v).nonzero()[:4].tolist())
    assert torch.equal(res.step_actions, ref.action.repeat_interleave(R, dim=0))
    assert len(torch.unique(ref.cand_score)) > G and not torch.equal(ref.probs, p0)
    small.close()
    big.close()


def test_one_call_of_three_iterations_equals_three_calls_of_one():
    import torch
    G, R, K, E, I = 5, 13, 4, 3, 3
    a, _ = _grouped(G, R)
    b, _ = _grouped(G, R)
    p0, s0 = _gprobs(K, G), _gseq(K, G)
    kw = dict(seed=77, draw=3, alpha=0.3, p_min=0.02, **OBJ)
    whole = a.plan_cem_groups(R, K, I, E, probs=p0.clone(), best_seq=s0.clone(), iter0=0, **kw)
    probs, seq, rows, cands = p0.clone(), s0.clone(), [], []
    for it in range(I):
        before_p, before_s = probs.clone(), seq.clone()
        r = b.plan_cem_groups(R, K, 1, E, probs=probs, best_seq=seq, iter0=it, **kw)
        assert r.probs is probs and r.best_seq is seq      # (updated in place and returned)
        assert np.array_equal(r.cand.cpu().numpy(), _sample_ref(before_p, before_s, R, 77, 3, it)), it
        rows.append(r.best_score[0].clone())
        cands.append(r.cand.clone())
    assert torch.equal(whole.best_score, torch.stack(rows))
    _same(whole, r, "the last of three calls", fields=("action", "step_actions", "best_seq", "probs", "cand", "cand_score"))
    assert not torch.equal(cands[0], cands[1]) and not torch.equal(cands[1], cands[2]) and not torch.equal(whole.probs, p0)
    # the incumbent's score never falls; a group's replicas hold one state, so equal sequences score equal
    for i in range(I - 1):
        assert bool((whole.best_score[i + 1] >= whole.best_score[i]).all()), i
    assert torch.equal(whole.cand_score[::R], whole.best_score[I - 2])      # (replica 0 played the incumbent of the iteration before)
    a.close()
    b.close()


def test_the_engine_afterwards():
    import torch
    G, R, K, E, I = 5, 13, 4, 3, 2
    b, g = _grouped(G, R)
    twin, _ = _grouped(G, R)
    kernel = b.last_step_kernel()
    kept, before = _outputs(b), _grab(b)
    left = b.steps_to_episode_end()
    res = b.plan_cem_groups(R, K, I, E, seed=2, alpha=0.3, p_min=0.02, **OBJ)
    assert res.best_score.shape == (I, G)
    _assert_rewound(b, before, "after plan_cem_groups")
    assert b.steps_to_episode_end() == left
    for nm, x in kept.items():
        assert torch.equal(getattr(b, nm).view(torch.uint8), x.view(torch.uint8)), nm
    x = _acts(G * R, g)
    twin.step(x)
    b.step(x)
    for nm in ("obs", "share_obs", "rew", "done"):
        assert torch.equal(getattr(b, nm), getattr(twin, nm)), nm
    assert b.last_step_kernel() == kernel == twin.last_step_kernel()
    # the call used up the envs' one live mark
    mk = b.mark(max_steps=4)
    b.plan_cem_groups(R, 2, 1, 1)
    with pytest.raises(ValueError, match="dead"):
        b.rewind(mk)
    b.close()
    twin.close()


def test_replicas_stay_in_sync_over_three_decisions():
    import torch
    G, R, K, E = 5, 13, 4, 3
    b, _ = _grouped(G, R)
    lead = torch.arange(G * R, device=b.device) // R * R
    assert torch.equal(b.obs, b.obs[lead]) and torch.equal(b.share_obs, b.share_obs[lead])
    probs = seq = None
    for d in range(3):
        res = b.plan_cem_groups(R, K, 2, E, probs=probs, best_seq=seq, seed=8, draw=d, alpha=0.3, p_min=0.02, **OBJ)
        assert torch.equal(res.step_actions, res.action[torch.arange(G * R, device=b.device) // R])
        # replicas that played one sequence from one state scored the same: replica 0 and every later copy of the incumbent
        b.step(res.step_actions)
        for nm in ("obs", "share_obs", "rew", "done", "info"):
            u = getattr(b, nm).clone()
            if nm == "info":
                u[:, RSV] = 0
            assert torch.equal(u, u[lead]), (d, nm, (u != u[lead]).nonzero()[:4].tolist())
        probs, seq = GroupCEMMPCAgent.shifted(res.probs, res.best_seq, K)
    assert len(torch.unique(b.obs[::R], dim=0)) == G      # (the groups themselves differ)
    b.close()


def test_chunked_output_block_gives_the_unchunked_results():
    G, R, K, E, I = 5, 13, 3, 3, 2
    whole, _ = _grouped(G, R)
    chunked, _ = _grouped(G, R, debug_flags=L.PLAN_DEBUG_TWO_STEPS)      # (chunks of 2 + 1 steps)
    kw = dict(probs=None, best_seq=None, seed=9, alpha=0.3, p_min=0.02, **OBJ)
    _same(whole.plan_cem_groups(R, K, I, E, **kw), chunked.plan_cem_groups(R, K, I, E, **kw), "chunked against whole")
    whole.close()
    chunked.close()


def test_refusals_leave_the_engine_untouched():
    import torch
    n, R = 8, 4
    a, split, fresh, verify, late = refusal_engines(n, alongside=1)
    mask = np.zeros(n, dtype=np.uint8)
    mask[5] = 1
    split.reset(mask=mask)      # env 5 starts a new episode: group 1 is out of step

    # what sdc_plan / sdc_plan_cem refuse
    planner_refusals(lambda e, K, **kw: e.plan_cem_groups(R, K, 1, 1, **kw), "n_steps", a, fresh, verify, late)
    refused(a, "n_steps", lambda: a.plan_cem_groups(R, 0, 1, 1))
    refused(a, "n_iters", lambda: a.plan_cem_groups(R, 3, 0, 1))
    refused(a, "iter0", lambda: a.plan_cem_groups(R, 3, 1, 1, iter0=-1))
    refused(a, "iter0", lambda: a.plan_cem_groups(R, 3, 2, 1, iter0=65535))
    refused(a, "fixed_action", lambda: a.plan_cem_groups(R, 3, 1, 2, fixed_action=(-1, 3, -1)))
    refused(a, "fixed_action", lambda: a.plan_cem_groups(R, 3, 1, 2, fixed_action=(-2, 0, 0)))
    refused(a, "three integers", lambda: a.plan_cem_groups(R, 3, 1, 2, fixed_action=(-1, -1)))
    for bad in (1.0, -0.1, float("nan")):
        refused(a, "alpha", lambda: a.plan_cem_groups(R, 3, 1, 2, alpha=bad))
    for bad in (0.34, -0.01, float("nan")):
        refused(a, "p_min", lambda: a.plan_cem_groups(R, 3, 1, 2, p_min=bad))
    # the groups
    refused(a, "group_size", lambda: a.plan_cem_groups(1, 3, 1, 1))
    refused(a, "group_size", lambda: a.plan_cem_groups(0, 3, 1, 1))
    refused(a, "group_size", lambda: a.plan_cem_groups(L.CEM_MAX_GROUP + 1, 3, 1, 1))
    refused(a, "not a multiple", lambda: a.plan_cem_groups(3, 3, 1, 1))
    refused(a, "not a multiple", lambda: a.plan_cem_groups(16, 3, 1, 1))
    refused(a, "n_elite", lambda: a.plan_cem_groups(R, 3, 1, 0))
    refused(a, "n_elite", lambda: a.plan_cem_groups(R, 3, 1, R + 1))
    refused(a, "group_base", lambda: a.plan_cem_groups(R, 3, 1, 1, group_base=-1))
    refused(split, "out of step.*env 5.*episode step", lambda: split.plan_cem_groups(R, 3, 1, 1))
    refused(split, "group_size", lambda: split.sync_groups(3))
    # malformed tensors
    G = n // R
    third = torch.full((3, G, 3, 3), 1.0 / 3.0, dtype=torch.float64, device=a.device)
    seq = torch.ones((3, G, 3), dtype=torch.int32, device=a.device)
    refused(a, "probs must be", lambda: a.plan_cem_groups(R, 3, 1, 2, probs=third.float()))
    refused(a, "probs must be", lambda: a.plan_cem_groups(R, 3, 1, 2, probs=third[:2]))
    refused(a, "probs must be", lambda: a.plan_cem_groups(R, 3, 1, 2, probs=third.cpu()))
    refused(a, "probs must be", lambda: a.plan_cem_groups(R, 3, 1, 2, probs=torch.full((3, n, 3, 3), 1.0 / 3.0, dtype=torch.float64, device=a.device)))
    refused(a, "best_seq must be", lambda: a.plan_cem_groups(R, 3, 1, 2, best_seq=seq.long()))
    refused(a, "best_seq must be", lambda: a.plan_cem_groups(R, 3, 1, 2, best_seq=torch.ones((6, G, 3), dtype=torch.int32, device=a.device)[::2]))
    # what the Python surface cannot send: straight to the library
    arrays = [third.clone(), seq.clone(), torch.empty((1, G), dtype=torch.float64, device=a.device),
              torch.empty((G, 3), dtype=torch.int32, device=a.device), torch.empty((n, 3), dtype=torch.int32, device=a.device),
              torch.empty((3, n, 3), dtype=torch.int32, device=a.device), torch.empty((n,), dtype=torch.float64, device=a.device)]
    p = lambda t: C.c_void_p(t.data_ptr())

    def params():
        c = L.SdcCemGroupParams()
        c.group_size, c.group_base, c.n_iters, c.iter0, c.n_elite, c.draw, c.seed, c.alpha, c.p_min = R, 0, 1, 0, 2, 0, 0, 0.0, 0.0
        c.fixed_action[:] = [-1, -1, -1]
        return c

    def raw(null=None, cem=params(), obj=None, no_cem=False):
        ptrs = [None if i == null else p(t) for i, t in enumerate(arrays)]
        rc = a.lib.sdc_plan_cem_groups(a._h, 3, None if no_cem else C.byref(cem), C.byref(obj) if obj is not None else None, *ptrs,
                                       p(a.obs), p(a.share_obs), a._stream())
        a._refused(rc)

    for i in range(len(arrays)):
        refused(a, "null array", lambda: raw(null=i))
    refused(a, "null cem", lambda: raw(no_cem=True))
    refused(a, "n_cols", lambda: raw(obj=objective(L.PLAN_MAX_COLS + 1, 0)))
    refused(a, "info column", lambda: raw(obj=objective(1, L.INFO_DIM)))
    # ... and the calls next to them go through: a NULL objective is the default one; the bounds themselves; a group put back in step
    raw()
    torch.cuda.synchronize()
    ok = a.plan_cem_groups(R, 3, 1, 2, probs=third.clone(), best_seq=seq.clone())
    assert torch.equal(arrays[6], ok.cand_score) and torch.equal(arrays[0], ok.probs) and torch.equal(arrays[4], ok.step_actions)
    assert a.plan_cem_groups(2, 37, 1, 2, iter0=65535, alpha=0.999, p_min=1.0 / 3.0).best_score.shape == (1, 4) and a.steps_to_episode_end() == 38
    assert a.plan_cem_groups(n, 2, 1, n, fixed_action=(2, 0, -1)).cand.shape == (2, n, 3)
    assert late.plan_cem_groups(R, 2, 2, 1).cand.shape == (2, n, 3) and late.steps_to_episode_end() == 2
    split.sync_groups(R)
    assert split.plan_cem_groups(R, 3, 1, 1).action.shape == (G, 3)
    for e in (a, fresh, verify, late, split):
        e.close()


def test_agent_across_an_auto_reset():
    import torch
    G, R, ep = 3, 6, 12
    N = G * R
    b = _mk(N, ep=ep, seed=7)
    ag = GroupCEMMPCAgent(R, n_elite=2, n_iters=2, horizon=4, seed=4, alpha=0.3, p_min=0.02, **OBJ)
    lead = torch.arange(N, device=b.device) // R * R
    starts = []      # (episode step, whether the decision started afresh) of every plan the agent asks for
    plan = b.plan_cem_groups
    b.plan_cem_groups = lambda *x, **kw: (starts.append((ep - b.steps_to_episode_end(), kw["probs"] is None and kw["best_seq"] is None)),
                                          plan(*x, **kw))[1]
    assert not torch.equal(b.obs, b.obs[lead])      # the replicas drew resets of their own
    planned = 0
    for t in range(ep + 3):
        step = ep - b.steps_to_episode_end()
        was = b.obs.clone()
        x = ag.act(b)
        assert x.shape == (N, 3) and x.dtype == torch.int32 and torch.equal(x, x[lead]), t
        if step == 0:      # a new episode: the groups were out of sync and have been re-synchronised before the plan
            assert not torch.equal(was, was[lead]) and torch.equal(b.obs, b.obs[lead]) and torch.equal(b.obs[lead], was[lead]), t
            assert starts[-1] == (0, True), (t, starts[-1])
        if ag.last is not None:
            planned += 1
            s = ag.last.best_score
            assert bool((s[1] >= s[0]).all()), t      # the incumbent's score never falls within a decision
            assert torch.equal(x, ag.last.step_actions)
        else:
            assert step == ep - 1 and bool((x == torch.tensor([1, 1, 2], dtype=torch.int32, device=b.device)).all())
        b.step(x)
        if step < ep - 1:      # inside an episode a group's replicas step as one (the terminal step resets each on its own)
            for nm in ("obs", "share_obs", "rew", "done", "info"):
                u = getattr(b, nm).clone()
                if nm == "info":
                    u[:, RSV] = 0
                assert torch.equal(u, u[lead]), (t, nm)
    assert ag.syncs == 2 and planned == ep + 3 - 1 and ag.draw == planned
    assert [s for s, fresh in starts if fresh] == [0, 0] and len(starts) == planned
    b.close()


def test_vec_env_plan_cem_groups_with_an_agent_subset():
    import torch
    n, R = 16, 4
    args = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True,
            "agents": ["agent_dc", "agent_bat"]}
    a = SustainDCVecEnv(args, n_envs=n, seed=3, months=[6] * n, return_torch=True)
    with pytest.raises(ValueError, match="reset"):
        a.plan_cem_groups(R, 3, 1, 2)
    a.reset()
    ag = GroupCEMMPCAgent(R, n_elite=2, n_iters=2, horizon=4, seed=4, alpha=0.3, p_min=0.02, reward_weights=(0.0, 1.0, 1.0), gamma=0.9,
                          info_weights={"bat_CO2_footprint": -1e-3})
    lead = torch.arange(n, device=a.engine.device) // R * R
    for t in range(4):
        x = ag.act(a)
        r = ag.last
        assert x.shape == (n, 2) and x.dtype == torch.int32 and torch.equal(x, r.step_actions)
        assert r.action.shape == (n // R, 2) and torch.equal(x, r.action[lead // R])
        assert torch.equal(r.action, r.best_seq[0][:, 1:])      # `action` comes back in the subset's columns
        sampled = r.cand.view(4, n // R, R, 3)[:, :, 1:]
        assert bool((sampled[..., 0] == 1).all())      # the slot outside the subset carries 1 in every sampled replica
        assert len(torch.unique(sampled[..., 1:])) == 3
        assert torch.equal(r.probs[:, :, 0], torch.full((4, n // R, 3), 1.0 / 3.0, dtype=torch.float64, device=r.probs.device))
        assert bool((r.best_score[1] >= r.best_score[0]).all())
        obs = a.step(x)[0]
        assert torch.equal(obs, obs[lead]), t
    assert ag.syncs == 1 and ag.draw == 4
    a.close()
