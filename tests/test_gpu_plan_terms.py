"""Plan terms (SdcEngine.set_plan_terms over sdc_set_plan_terms: limits on info columns and a terminal term in the planners' score)
held to the stated arithmetic (include/sustaindc_hip.h) restated in torch fp64 from a twin engine's rollouts.

 1. sdc_plan's scores bit for bit against the restatement at 164 envs (two full workgroups and one whose second half-tile holds 4
    rows), with 2 limits + 1 terminal column and with all 8 + 8 slots, the bounds the medians of the twin's own rollouts;  2. no terms,
    terms set and cleared, and both counts 0 all give the bits of a plan that never saw terms;  3. the chunked output block (debug_flags
    PLAN_DEBUG_TWO_STEPS, chunks of 2 + 2 + 1 steps: the terminal step alone in the last) against the unchunked one;  4. the selection follows the
    terms;  5. plan_cem and plan_cem_groups score with them;  6. the refusals, each of which leaves the terms and the engine as they
    were;  7. the vector env, and copy.deepcopy of it and of SustainDC.

Not in verify mode, episodes of 96 steps and rings of 128 keys, as in tests/test_gpu_plan.py."""
import copy
import ctypes as C

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import SustainDC, SustainDCVecEnv
from tests.plan_util import RSV, _twins, refused
from tests.test_gpu_mark import _assert_rewound, _grab, _mk
from tests.test_gpu_plan import _cands, _objective, _pz

pytestmark = pytest.mark.gpu

W, GAMMA = (0.5, 2.0, -1.0), 0.9
COLS = {L.INFO_COLS[0]: 0.25, "bat_CO2_footprint": -1e-3, "energy_z": 3.0}      # the objective's own three columns
I = L.INFO_IDX


def _entries(limits):
    """set_plan_terms' `limits` dict -> the library's entries (key, side, bound, weight): each side given, in dict order, low first"""
    return [(k, side, b, w) for k, (lo, hi, w) in limits.items() for side, b in ((-1, lo), (1, hi)) if b is not None]


def _terms_objective(rew, info, w, gamma, cols, limits, terminal):
    """sdc_plan's arithmetic with plan terms (include/sustaindc_hip.h sdc_set_plan_terms) from one candidate's rew [K, N, 3] / info
    [K, N, 44]: element-wise fp64 multiplies, adds and subtractions in the stated order, the hinge a compare and a select -> score [N]"""
    import torch
    K, N = rew.shape[0], rew.shape[1]
    score = torch.zeros((N,), dtype=torch.float64, device=rew.device)
    zero = torch.zeros((N,), dtype=torch.float64, device=rew.device)
    gk = 1.0
    for k in range(K):
        if k:
            gk = gk * gamma
        r = rew[k].double()
        s = (r[:, 0] * w[0] + r[:, 1] * w[1]) + r[:, 2] * w[2]
        for key, cw in cols.items():
            s = s + info[k][:, I[key]].double() * cw
        for key, side, bound, lw in _entries(limits):
            x = info[k][:, I[key]].double()
            d = x - bound if side > 0 else bound - x
            e = torch.where(d > 0.0, d, zero)
            s = s - e * lw
        score = score + s * gk
    t = zero.clone()
    for key, tw in terminal.items():
        t = t + info[K - 1][:, I[key]].double() * tw
    if terminal:
        score = score + t * (gk * gamma)
    return score


def _rollouts(twin, cand):
    """the launches a plan takes, on the twin: mark, then per candidate a rollout and a rewind -> [(rew [K, N, 3], info [K, N, 44])]"""
    mk = twin.mark(max_steps=int(cand.shape[1]))
    outs = []
    for c in range(int(cand.shape[0])):
        o = twin.rollout(cand[c])
        outs.append((o[2].clone(), o[4].clone()))
        twin.rewind(mk)
    return outs


def _median(outs, key):
    """the column's median over candidate 0's K x N values, as a Python float (an fp32 value: exact)"""
    return float(outs[0][1][:, :, I[key]].flatten().median())


def test_scores_bit_for_bit_against_the_restatement():
    import torch
    N, M, K = 164, 2, 7
    (b, twin), g = _twins(N)
    cand = _cands(M, K, N, g)
    outs = _rollouts(twin, cand)
    med = lambda key: _median(outs, key)
    few = (
        {"dc_int_temperature": (None, med("dc_int_temperature"), 0.75), "dc_total_power_kW": (med("dc_total_power_kW"), None, 1e-3)},
        {"ls_tasks_in_queue": -0.5},
    )
    uppers = ["dc_int_temperature", "dc_ITE_total_power_kW", "dc_water_usage", "norm_CI"]
    lowers = ["dc_total_power_kW", "dc_HVAC_total_power_kW", "bat_CO2_footprint", "outside_temp"]
    full_limits = {}
    for j, (u, lo) in enumerate(zip(uppers, lowers)):      # upper and lower sides alternate
        full_limits[u] = (None, med(u), 0.5 + j)
        full_limits[lo] = (med(lo), None, 1e-3 * (j + 1))
    full = (full_limits, {"ls_tasks_in_queue": -0.5, "ls_oldest_task_age": -0.25, "bat_SOC": 2.0, "ls_overdue_penalty": -1.0,
                          "ls_norm_tasks_in_queue": -3.0, "dc_int_temperature": -0.125, "bat_CO2_footprint": -1e-4, "energy_z": 0.5})
    assert len(_entries(full[0])) == L.PLAN_MAX_LIMITS and len(full[1]) == L.PLAN_MAX_TERMINAL
    assert RSV not in [I[k] for k in list(full[0]) + list(full[1]) + list(COLS)]
    plain = b.plan(cand, reward_weights=W, gamma=GAMMA, info_weights=COLS)
    for limits, terminal in (few, full):
        # every bound splits the twin's env-steps: some exceed it, some do not
        for key, side, bound, _ in _entries(limits):
            x = torch.stack([o[1][:, :, I[key]] for o in outs]).double()
            over = (x - bound > 0.0) if side > 0 else (bound - x > 0.0)
            assert bool(over.any()) and not bool(over.all()), (key, side, bound)
        b.set_plan_terms(limits, terminal)
        assert b.plan_terms == (limits, terminal)
        res = b.plan(cand, reward_weights=W, gamma=GAMMA, info_weights=COLS)
        for c in range(M):
            score = _terms_objective(outs[c][0], outs[c][1], W, GAMMA, COLS, limits, terminal)
            assert torch.equal(_pz(res.score[c]), _pz(score)), (len(terminal), c, (res.score[c] - score).abs().max().item())
            returns, untermed = _objective(outs[c][0], outs[c][1], W, GAMMA, COLS)
            assert torch.equal(_pz(res.returns[c]), _pz(returns)), (len(terminal), c, "returns")
            assert torch.equal(_pz(plain.score[c]), _pz(untermed)), (c, "the plain plan")
        assert torch.equal(res.returns, plain.returns) and not torch.equal(res.score, plain.score)
    # without the objective's own columns, and with the terminal term alone (no limits)
    b.set_plan_terms(terminal=few[1])
    res = b.plan(cand, reward_weights=W, gamma=GAMMA)
    for c in range(M):
        score = _terms_objective(outs[c][0], outs[c][1], W, GAMMA, {}, {}, few[1])
        assert torch.equal(_pz(res.score[c]), _pz(score)), (c, "terminal alone")
    b.close()
    twin.close()


def test_no_terms_means_the_plain_plan_to_the_bit():
    import torch
    N, M, K = 130, 3, 5
    (b,), g = _twins(N, n=1)
    cand = _cands(M, K, N, g)
    kw = dict(reward_weights=W, gamma=GAMMA, info_weights=COLS)
    before = _grab(b)
    first = b.plan(cand, **kw)
    _assert_rewound(b, before, "after the plain plan")
    b.set_plan_terms({"dc_int_temperature": (None, 20.0, 1.0)}, {"bat_SOC": 1.0})
    termed = b.plan(cand, **kw)
    assert not torch.equal(termed.score, first.score)
    _assert_rewound(b, before, "after the plan with terms")
    b.set_plan_terms()
    assert b.plan_terms == ({}, {})
    cleared = b.plan(cand, **kw)
    # both counts 0 clears, whatever the other fields hold
    b.set_plan_terms({"dc_int_temperature": (None, 20.0, 1.0)})
    s = L.SdcPlanTerms()
    s.limit_col[0], s.limit_side[0], s.limit_bound[0], s.terminal_col[0] = 99, 7, float("nan"), -3
    b._set_plan_terms_struct(s)
    assert b.plan_terms == ({}, {})
    zero = b.plan(cand, **kw)
    for res, what in ((cleared, "set and cleared"), (zero, "both counts 0")):
        for nm in ("score", "returns", "best", "action"):
            u, v = getattr(res, nm), getattr(first, nm)
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), (what, nm)
    _assert_rewound(b, before, "after the last plan")
    b.close()


def test_chunked_output_block_gives_the_unchunked_results():
    import torch
    N, M, K = 130, 3, 5
    whole = _twins(N, n=1)[0][0]
    (chunked,), g = _twins(N, n=1, debug_flags=L.PLAN_DEBUG_TWO_STEPS)      # (chunks of 2 + 2 + 1 steps: the terminal step alone)
    cand = _cands(M, K, N, g)
    kw = dict(reward_weights=(1.0, 0.5, 2.0), gamma=0.95, info_weights={"bat_CO2_footprint": -1e-3})
    plain = whole.plan(cand, **kw)
    for e in (whole, chunked):
        e.set_plan_terms({"dc_int_temperature": (18.0, 22.0, 0.5), "dc_crac_setpoint": (None, 20.0, 2.0)},
                         {"ls_tasks_in_queue": -0.5, "bat_SOC": 2.0})
    ra, rb = whole.plan(cand, **kw), chunked.plan(cand, **kw)
    for nm in ("returns", "score", "best", "action"):
        assert torch.equal(getattr(ra, nm).view(torch.uint8), getattr(rb, nm).view(torch.uint8)), nm
    assert not torch.equal(ra.score, plain.score)
    # the terminal term alone separates the two as well: it is applied once, in the last chunk
    for e in (whole, chunked):
        e.set_plan_terms(terminal={"ls_tasks_in_queue": -0.5, "bat_SOC": 2.0})
    ta, tb = whole.plan(cand, **kw), chunked.plan(cand, **kw)
    assert torch.equal(ta.score.view(torch.uint8), tb.score.view(torch.uint8))
    assert not torch.equal(ta.score, plain.score) and not torch.equal(ta.score, ra.score)
    whole.close()
    chunked.close()


def test_selection_follows_the_terms():
    import torch
    N, K = 130, 6
    (b, twin), _ = _twins(N)
    cand = torch.ones((2, K, N, 3), dtype=torch.int32, device=b.device)
    cand[..., 2] = 2                # (ls 1, bat 2: do nothing)
    cand[0, :, :, 1] = 0            # candidate 0 lowers the CRAC set point every step,
    cand[1, :, :, 1] = 2            # candidate 1 raises it
    col = I["dc_crac_setpoint"]
    # one bound serves the whole batch: the median over the envs of the set point before the plan
    bound = float(b.info[:, col].median())
    outs = _rollouts(twin, cand)
    assert bool((outs[1][1][:, :, col] > outs[0][1][:, :, col]).any())      # (the candidates do what they are called)
    plain = b.plan(cand)
    unlimited = [_objective(r, i, (1.0, 1.0, 1.0), 1.0, {})[1] for r, i in outs]
    plain_best = (unlimited[1] > unlimited[0]).to(torch.int32)      # (candidate 0 unless candidate 1 is strictly better)
    assert torch.equal(plain.best, plain_best)
    # An upper limit punishes the candidate that raises, a lower limit the one that lowers.  The limit that can change a choice is the
    # one against the candidate the plain objective prefers: upper where some env prefers raising (what the default rewards do: a
    # higher set point saves cooling energy), lower only if every env prefers lowering
    limits = {"dc_crac_setpoint": (None, bound, 1e6) if bool((plain_best == 1).any()) else (bound, None, 1e6)}
    b.set_plan_terms(limits)
    res = b.plan(cand)
    scores = torch.stack([_terms_objective(r, i, (1.0, 1.0, 1.0), 1.0, {}, limits, {}) for r, i in outs])
    assert torch.equal(_pz(res.score), _pz(scores))
    want = (scores[1] > scores[0]).to(torch.int32)
    assert torch.equal(res.best, want)
    flipped = int((res.best != plain.best).sum())
    assert flipped >= 1, "the limit changed no env's choice"
    assert torch.equal(res.action, cand[res.best.long(), 0, torch.arange(N, device=b.device)])
    b.close()
    twin.close()


TERMS = ({"dc_int_temperature": (None, 21.0, 0.75), "dc_crac_setpoint": (19.0, 21.0, 2.0)}, {"ls_tasks_in_queue": -0.5, "bat_SOC": 2.0})


def test_plan_cem_scores_with_the_terms():
    import torch
    N, M, K, IT = 130, 4, 4, 2
    (b, twin), _ = _twins(N)
    kw = dict(seed=7, draw=1, reward_weights=W, gamma=GAMMA, info_weights=COLS)
    plain = b.plan_cem(K, IT, M, 2, **kw)
    b.set_plan_terms(*TERMS)
    res = b.plan_cem(K, IT, M, 2, **kw)
    outs = _rollouts(twin, res.cand)
    for c in range(M):
        score = _terms_objective(outs[c][0], outs[c][1], W, GAMMA, COLS, *TERMS)
        assert torch.equal(_pz(res.cand_score[c]), _pz(score)), (c, (res.cand_score[c] - score).abs().max().item())
    assert not torch.equal(res.cand_score[0], plain.cand_score[0])      # (the incumbents' scores)
    b.close()
    twin.close()


def test_plan_cem_groups_equals_plan_cem_with_the_same_terms():
    import torch
    G, R, K, IT, E = 8, 4, 4, 2, 2
    (small,), _ = _twins(G, n=1)
    big = _mk(G * R, ep=96, seed=33)
    big.restore(small.snapshot(), envs=np.arange(G * R), rows=np.arange(G * R) // R)      # group g holds the small engine's env g
    kw = dict(seed=99, draw=4, alpha=0.3, p_min=0.02, reward_weights=W, gamma=GAMMA, info_weights=COLS)
    plain = big.plan_cem_groups(R, K, IT, E, group_base=0, **kw)
    for e in (small, big):
        e.set_plan_terms(*TERMS)
    ref = small.plan_cem(K, IT, R, E, **kw)
    res = big.plan_cem_groups(R, K, IT, E, group_base=0, **kw)
    score = res.cand_score.view(G, R).t().contiguous()      # [R, G]: replica r of group g is candidate r of env g
    assert torch.equal(score.view(torch.uint8), ref.cand_score.view(torch.uint8)), (score - ref.cand_score).abs().max().item()
    for nm in ("probs", "best_seq", "best_score", "action"):
        assert torch.equal(getattr(res, nm), getattr(ref, nm)), nm
    assert not torch.equal(res.cand_score.view(G, R)[:, 0], plain.cand_score.view(G, R)[:, 0])
    small.close()
    big.close()


def test_refusals_leave_the_terms_and_the_engine_as_they_were():
    import torch
    N = 8
    (a,), g = _twins(N, n=1, history=6)
    kept = ({"dc_int_temperature": (None, 27.0, 10.0), "bat_SOC": (0.2, None, 5.0)}, {"ls_tasks_in_queue": -1.0})
    a.set_plan_terms(*kept)
    cand = _cands(2, 3, N, g)
    before = a.plan(cand).score

    def good():
        s = L.SdcPlanTerms()
        s.n_limits, s.n_terminal = 2, 1
        s.limit_col[0], s.limit_side[0], s.limit_bound[0], s.limit_weight[0] = 3, 1, 1.0, 1.0
        s.limit_col[1], s.limit_side[1], s.limit_bound[1], s.limit_weight[1] = 4, -1, 2.0, 0.0
        s.terminal_col[0], s.terminal_weight[0] = 5, -1.0
        return s

    def bad(match, **fields):
        s = good()
        for name, value in fields.items():
            if isinstance(value, tuple):
                getattr(s, name)[value[0]] = value[1]
            else:
                setattr(s, name, value)
        refused(a, match, lambda: a._set_plan_terms_struct(s))
        assert a.plan_terms == kept, match

    a._set_plan_terms_struct(good())      # (the struct the bad ones are made from goes through)
    a.set_plan_terms(*kept)
    bad("n_limits", n_limits=L.PLAN_MAX_LIMITS + 1)
    bad("n_limits", n_limits=-1)
    bad("n_terminal", n_terminal=L.PLAN_MAX_TERMINAL + 1)
    bad("n_terminal", n_terminal=-1)
    bad(r"limit_col\[1\]", limit_col=(1, L.INFO_DIM))
    bad(r"limit_col\[0\]", limit_col=(0, -1))
    bad(r"terminal_col\[0\]", terminal_col=(0, L.INFO_DIM))
    bad(r"terminal_col\[0\]", terminal_col=(0, -1))
    for side in (0, 2, -2):
        bad(r"limit_side\[1\]", limit_side=(1, side))
    for x in (float("inf"), float("-inf"), float("nan")):
        bad(r"limit_bound\[0\]", limit_bound=(0, x))
        bad(r"limit_weight\[1\]", limit_weight=(1, x))
        bad(r"terminal_weight\[0\]", terminal_weight=(0, x))
    bad(r"limit_weight\[0\].*negative", limit_weight=(0, -0.5))
    # a null handle: from the library itself
    assert a.lib.sdc_set_plan_terms(None, C.byref(good())) == -2 and b"null handle" in a.lib.sdc_last_error()
    assert a.plan_terms == kept
    # what the Python surface refuses itself, and what it hands on
    refused(a, "limits key 'no_such_key' is not an info column", lambda: a.set_plan_terms({"no_such_key": (0.0, 1.0, 1.0)}))
    refused(a, "terminal key 'no_such_key' is not an info column", lambda: a.set_plan_terms(terminal={"no_such_key": 1.0}))
    refused(a, "at most 8", lambda: a.set_plan_terms({k: (0.0, 1.0, 1.0) for k in L.INFO_COLS[:5]}))      # (10 entries)
    refused(a, "at most 8", lambda: a.set_plan_terms(terminal={k: 1.0 for k in L.INFO_COLS[:9]}))
    refused(a, r"\(low, high, weight\)", lambda: a.set_plan_terms({"bat_SOC": (0.2, 1.0)}))
    refused(a, "limit_weight.*negative", lambda: a.set_plan_terms({"bat_SOC": (0.2, None, -1.0)}))
    refused(a, "limit_bound.*not finite", lambda: a.set_plan_terms({"bat_SOC": (float("nan"), None, 1.0)}))
    refused(a, "terminal_weight.*not finite", lambda: a.set_plan_terms(terminal={"bat_SOC": float("inf")}))
    assert a.plan_terms == kept
    assert torch.equal(a.plan(cand).score.view(torch.uint8), before.view(torch.uint8))      # the terms in force score as before
    a.close()


def test_vec_env_and_deepcopy_carry_the_terms():
    import torch
    N, M, K = 16, 3, 4
    args = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True}
    a = SustainDCVecEnv(args, n_envs=N, seed=3, months=[6] * N, return_torch=True)
    b = SustainDCVecEnv(args, n_envs=N, seed=3, months=[6] * N, return_torch=True)
    a.set_plan_terms(*TERMS)      # (host state: before reset() as well)
    assert a.plan_terms == TERMS and b.plan_terms == ({}, {})
    a.reset()
    b.reset()
    rng = np.random.default_rng(2)
    for _ in range(5):
        x = torch.as_tensor(rng.integers(0, 3, (N, 3)).astype(np.int32), device=a.engine.device)
        a.step(x)
        b.step(x)
    cand = torch.as_tensor(rng.integers(0, 3, (M, K, N, 3)).astype(np.int32), device=a.engine.device)
    kw = dict(reward_weights=W, gamma=GAMMA, info_weights=COLS)
    plain = b.engine.plan(cand, **kw)
    b.engine.set_plan_terms(*TERMS)
    ra, rb = a.plan(cand, **kw), b.engine.plan(cand, **kw)
    cp = copy.deepcopy(a)
    assert cp.plan_terms == TERMS
    rc = cp.plan(cand, **kw)
    for nm in ("score", "returns", "best", "action"):
        assert torch.equal(getattr(ra, nm).view(torch.uint8), getattr(rb, nm).view(torch.uint8)), nm
        assert torch.equal(getattr(ra, nm).view(torch.uint8), getattr(rc, nm).view(torch.uint8)), ("deepcopy", nm)
    assert not torch.equal(ra.score, plain.score)
    a.set_plan_terms()
    assert a.plan_terms == ({}, {}) and cp.plan_terms == TERMS      # (the copy's terms are its own)
    for e in (a, b, cp):
        e.close()
    # SustainDC's deepcopy goes the same way
    env = SustainDC({"location": "ny", "month": 6, "days_per_episode": 1}, seed=4)
    env._vec.set_plan_terms(*TERMS)
    env.reset()
    twin = copy.deepcopy(env)
    assert twin._vec.plan_terms == TERMS
    env.close()
    twin.close()
