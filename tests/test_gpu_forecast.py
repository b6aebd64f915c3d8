"""Plan forecasts (SdcEngine.set_plan_forecast over sdc_set_plan_forecast; the kernels: csrc/sdc_forecast.hip) -- everything bit for bit.

 1. the fill kernel (`forecast_traces`, `future_traces`) against a NumPy restatement from the record, the tables and the weather
    windows, on a batch whose envs stand at different episode steps (both DAILY branches), every mode on every channel;
 2. a forecast is the future of another engine: twin B, whose tables and windows are rewritten so that its real future IS the forecast F
    (W, C at table indices i + j of the env's own location, T, WB at rel + j of its windows), plans without a forecast through the
    general kernel's in-step path (its rows are stale after the writes); A under the forecast must give B's score, returns, best and
    action -- on every step mapping and the chunked output block; once each for plan_cem and plan_cem_groups;
 3. nothing is left behind: snapshots of the whole batch (feature rows included) before and after a plan under a forecast, and after a
    refused one; a run that plans before every step equals a twin that only takes the chosen actions;
 4. the refusals;  5. cleared means absent, all-perfect means absent, copy.deepcopy carries the forecast.

Test 2 needs a table per env, i.e. one location per env, which tests/test_gpu_mark._mk does not build: `_mk_per_env` is _mk with the
"ny" tables under N location ids.  The other engines are _mk's.  Episodes of 96 steps, rings of 128 keys (tests/test_gpu_plan.py)."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import SustainDCVecEnv, traces
from dc_rl_amd.engine import SdcEngine
from tests.plan_util import EP, OBJ, RSV, _outputs, _twins, refused
from tests.test_gpu_clone import _acts
from tests.test_gpu_mark import _mk, _setup
from tests.test_gpu_plan import _cands

pytestmark = pytest.mark.gpu

R_CURSOR, R_TREL, R_LOC = 0, 1, 25      # csrc/sdc_device.hpp SdcRec
DAY = 96
ALL = lambda m: dict(workload=m, carbon=m, temperature=m, wet_bulb=m)


def _same(u, v):
    import torch
    return torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))


# ---- 1. the fill against NumPy ---------------------------------------------------------------------------------------------------------
def _fill_ref(rec, tabs, t_win, wb_win, modes, values, n):
    """include/sustaindc_hip.h sdc_set_plan_forecast restated: fc [n, N, 4] from the record, the tables per location, the windows"""
    i, rel, loc = (rec[:, c].astype(np.int64) for c in (R_CURSOR, R_TREL, R_LOC))
    N = rec.shape[0]
    env = np.arange(N)
    tix = lambda x: np.clip(x, 0, L.TABLE_LEN - 1)
    fc = np.empty((n, N, 4), dtype=np.float64)
    for j in range(n):
        for c, m in enumerate(modes):
            if m == L.FORECAST_VALUES:
                fc[j, :, c] = values[j, :, c]
                continue
            back = m == L.FORECAST_DAILY and j >= 1
            if c < 2:
                at = i if m == L.FORECAST_PERSISTENCE else i + j - DAY if back else i + j
                fc[j, :, c] = tabs[c][loc, tix(at)]
            else:
                at = rel if m == L.FORECAST_PERSISTENCE else np.where(rel + j >= DAY, rel + j - DAY, rel) if back else rel + j
                fc[j, :, c] = (t_win if c == 2 else wb_win)[env, at]
    return fc


def test_fill_kernel_against_numpy():
    import torch
    N, ep = 192, 192
    eng = _mk(N, mixed=True, ep=ep)
    g = torch.Generator(device="cpu").manual_seed(3)
    for _ in range(110):
        eng.step(_acts(N, g))
    eng.reset((np.arange(N) % 3 == 1).astype(np.uint8))
    for _ in range(10):
        eng.step(_acts(N, g))
    rec = eng.get_state("record")
    rel = rec[:, R_TREL].astype(np.int64)
    assert set(rel.tolist()) == {10, 120} and len(set(rec[:, R_LOC].tolist())) > 1
    tables = _setup(True)[2]
    tabs = [np.stack([tb[k] for tb in tables]).astype(np.float64) for k in ("W", "C")]
    t_win, wb_win = eng.get_state("t_win"), eng.get_state("wb_win")
    values = torch.rand((18, N, 4), dtype=torch.float64, generator=g).cuda()
    combos = [(m,) * 4 for m in range(4)] + [(1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2), (0, 1, 2, 3)]
    for n in (3, 18):
        truth = _fill_ref(rec, tabs, t_win, wb_win, (0, 0, 0, 0), None, n)
        for modes in combos:
            eng.set_plan_forecast(*modes, values=values if 3 in modes else None)
            want = _fill_ref(rec, tabs, t_win, wb_win, modes, values.cpu().numpy(), n)
            got = eng.forecast_traces(n).cpu().numpy()
            assert got.shape == (n, N, 4) and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, modes)
            assert np.array_equal(eng.future_traces(n).cpu().numpy().view(np.uint64), truth.view(np.uint64)), (n, modes, "truth")
        # both DAILY branches occurred, and they differ from persistence and from the truth
        daily = _fill_ref(rec, tabs, t_win, wb_win, (2, 2, 2, 2), None, n)
        pers = _fill_ref(rec, tabs, t_win, wb_win, (1, 1, 1, 1), None, n)
        assert np.array_equal(daily[:, rel == 10, 2:], pers[:, rel == 10, 2:]) and not np.array_equal(daily[:, rel == 120, 2:], pers[:, rel == 120, 2:])
        assert not np.array_equal(daily, truth) and not np.array_equal(pers, truth)
    eng.close()


# ---- 2. a forecast is the future of another engine -----------------------------------------------------------------------------------
N2, M2, K2 = 128, 5, 6
CEM = dict(seed=7, draw=2, alpha=0.2, p_min=0.01)


def _mk_per_env(N, seed=21, history=20, **kw):
    """_mk with one location per env (every location holds the "ny" tables), `history` random steps in"""
    import torch
    _, _, tables, params = _setup(False)
    eng = SdcEngine(N, episode_steps=EP, auto_reset=True, seed=seed, hist_cap=128, n_locations=N, n_dc_configs=len(params), **kw)
    tb = tables[0]
    for li in range(N):
        eng.set_tables(li, tb["W"], tb["C"], tb["T"], tb["WB"])
    for ci, p in enumerate(params):
        eng.set_dc_params(ci, p)
    init_day = traces.get_init_day(6)
    eng.assign(np.arange(N, dtype=np.int32), np.zeros(N, dtype=np.int32), init_day - 7, init_day + 7)
    eng.reset()
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(history):
        eng.step(_acts(N, g))
    return eng, g


class _Future:
    """engine B, whose future is rewritten to a forecast F [J, N, 4]: the tables of every env's location at i + j, its windows at rel + j"""

    def __init__(self, b):
        self.b = b
        rec = b.get_state("record")
        self.i, self.rel, self.loc = (rec[:, c].astype(np.int64) for c in (R_CURSOR, R_TREL, R_LOC))
        self.tb = {k: np.asarray(v, dtype=np.float64) for k, v in _setup(False)[2][0].items()}
        self.t_win, self.wb_win = b.get_state("t_win"), b.get_state("wb_win")

    def impose(self, F):
        F = F.cpu().numpy()
        J = F.shape[0]
        t_win, wb_win = self.t_win.copy(), self.wb_win.copy()
        assert int(self.i.max()) + J <= L.TABLE_LEN
        for n in range(self.b.n_envs):
            W, Cc = self.tb["W"].copy(), self.tb["C"].copy()
            W[self.i[n]:self.i[n] + J] = F[:, n, 0]
            Cc[self.i[n]:self.i[n] + J] = F[:, n, 1]
            self.b.set_tables(int(self.loc[n]), W, Cc, self.tb["T"], self.tb["WB"])
            t_win[n, self.rel[n]:self.rel[n] + J] = F[:, n, 2]
            wb_win[n, self.rel[n]:self.rel[n] + J] = F[:, n, 3]
        self.b.set_state("t_win", t_win)      # (host writes: B's feature rows are stale from here on, its steps compute from the tables)
        self.b.set_state("wb_win", wb_win)


def _noisy(truth, g):
    """a VALUES forecast: the truth with an error of its own on every channel, entry 0 the truth; workload kept inside [0, 1]"""
    import torch
    e = torch.randn(truth.shape, dtype=torch.float64, generator=g).to(truth.device)
    v = truth.clone()
    v[..., 0] = (truth[..., 0] + 0.05 * e[..., 0]).clamp(0.0, 1.0)
    v[..., 1] = truth[..., 1] * (1.0 + 0.1 * e[..., 1])
    v[..., 2:] = truth[..., 2:] + e[..., 2:]
    v[0] = truth[0]
    return v.contiguous()


@functools.lru_cache(maxsize=None)
def _reference():
    """once for all mappings: the candidates, the three forecasts taken from a default-mapping A, and B's plans without a forecast on the
    futures they describe (plan for each, plan_cem for persistence)"""
    a, g = _mk_per_env(N2)
    b, _ = _mk_per_env(N2)
    cand = _cands(M2, K2, N2, g)
    truth = a.future_traces(K2 + 2)
    F = {}
    a.set_plan_forecast(**ALL("persistence"))
    F["persistence"] = a.forecast_traces(K2 + 2)
    a.set_plan_forecast(carbon="daily")
    F["daily_carbon"] = a.forecast_traces(K2 + 2)
    F["values"] = _noisy(truth, g)
    for name, f in F.items():
        assert _same(f[0], truth[0]) and not _same(f, truth), name
    fut, plans = _Future(b), {}
    for name, f in F.items():
        fut.impose(f)
        r = b.plan(cand, **OBJ)
        plans[name] = {nm: getattr(r, nm).clone() for nm in ("score", "returns", "best", "action")}
    fut.impose(F["persistence"])
    r = b.plan_cem(K2, 2, 4, 2, **CEM, **OBJ)
    cem = {nm: getattr(r, nm).clone() for nm in ("best_seq", "best_score", "probs", "action")}
    a.close()
    b.close()
    return cand, F, plans, cem


def _set(eng, name, F):
    if name == "persistence":
        eng.set_plan_forecast(**ALL("persistence"))
    elif name == "daily_carbon":
        eng.set_plan_forecast(carbon="daily")
    else:
        eng.set_plan_forecast(**ALL("values"), values=F["values"])


MAPPINGS = {"default": 0, "quad": L.DEBUG_QUAD, "wide": L.DEBUG_WIDE, "general": L.DEBUG_GENERAL, "two_steps": L.PLAN_DEBUG_TWO_STEPS}


@pytest.mark.parametrize("mapping", list(MAPPINGS))
def test_plan_under_a_forecast_equals_a_twin_whose_future_it_is(mapping):
    cand, F, plans, _ = _reference()
    a, _ = _mk_per_env(N2, debug_flags=MAPPINGS[mapping])
    oracle = a.plan(cand, **OBJ)
    for name in F:
        _set(a, name, F)
        assert _same(a.forecast_traces(K2 + 2), F[name]), (mapping, name)      # (this mapping's A stands where the reference's stood)
        r = a.plan(cand, **OBJ)
        for nm, want in plans[name].items():
            got = getattr(r, nm)
            assert _same(got, want), (mapping, name, nm, int((got != want).sum()))
        assert not _same(r.score, oracle.score), (mapping, name, "the forecast changed no score")
    a.close()


def test_plan_cem_under_a_forecast_equals_the_twin():
    _, F, _, cem = _reference()
    a, _ = _mk_per_env(N2)
    _set(a, "persistence", F)
    r = a.plan_cem(K2, 2, 4, 2, **CEM, **OBJ)
    for nm, want in cem.items():
        assert _same(getattr(r, nm), want), nm
    a.close()


def test_plan_cem_groups_under_a_forecast_equals_the_twin():
    R = 4
    a, _ = _mk_per_env(N2)
    b, _ = _mk_per_env(N2)
    for e in (a, b):
        e.sync_groups(R)
    a.set_plan_forecast(**ALL("persistence"))
    f = a.forecast_traces(K2 + 2)
    assert _same(f.view(K2 + 2, N2 // R, R, 4)[:, :, 1:], f.view(K2 + 2, N2 // R, R, 4)[:, :, :1].expand(-1, -1, R - 1, -1))
    _Future(b).impose(f)
    kw = dict(group_base=0, **CEM, **OBJ)
    want, got = b.plan_cem_groups(R, K2, 2, 2, **kw), a.plan_cem_groups(R, K2, 2, 2, **kw)
    for nm in ("best_seq", "best_score", "probs", "action", "step_actions"):
        assert _same(getattr(got, nm), getattr(want, nm)), nm
    a.close()
    b.close()


# ---- 3. nothing is left behind -----------------------------------------------------------------------------------------------------------
def _snapshot_rows(eng):
    """SdcEngine.snapshot() of the whole batch into a ZEROED buffer -> its rows: a row's padding (behind the feature rows, up to the next
    256 bytes) is not written by the library, and what torch.empty leaves there differs from one snapshot to the next"""
    import torch
    from dc_rl_amd.engine import _ip, _p
    n = eng.n_envs
    rows = torch.zeros((n, int(eng.lib.sdc_snapshot_row_bytes(eng._h))), dtype=torch.uint8, device=eng.device)
    manifest = np.zeros((n, L.SNAPSHOT_MANIFEST), dtype=np.int32)
    eng._call(eng.lib.sdc_snapshot_envs, _ip(np.arange(n, dtype=np.int32)), n, _p(rows), _ip(manifest), *eng._obs_ptrs, eng._stream(), refuses=True)
    return rows


def test_the_rows_are_what_they_were_after_a_plan_and_after_a_refused_one():
    N, M, K = 130, 3, 5
    (a,), g = _twins(N, n=1)
    cand = _cands(M, K, N, g)
    before = _snapshot_rows(a)
    assert before.shape[1] > (EP + 1) * 128      # (the feature rows are in there)
    a.set_plan_forecast(**ALL("persistence"))
    a.plan(cand, **OBJ)
    assert _same(before, _snapshot_rows(a))
    a.set_plan_forecast(workload="values")      # no values: refused
    with pytest.raises(ValueError, match="values is null"):
        a.plan(cand, **OBJ)
    a.set_plan_forecast(**ALL("daily"))
    with pytest.raises(ValueError, match="gamma"):
        a.plan(cand, gamma=2.0)
    assert _same(before, _snapshot_rows(a))
    # ... and the overlay was there in between: the same plan without a forecast scores otherwise
    under = a.plan(cand, **OBJ)
    a.set_plan_forecast(None)
    assert not _same(under.score, a.plan(cand, **OBJ).score) and _same(before, _snapshot_rows(a))
    a.close()


def test_planning_under_a_forecast_before_every_step_does_not_change_the_run():
    import torch
    N, M, K = 64, 3, 4
    (a, b), g = _twins(N)
    a.set_plan_forecast(workload="persistence", carbon="daily", temperature="persistence", wet_bulb="daily")
    keep = [c for c in range(L.INFO_DIM) if c != RSV]
    for step in range(30):
        action = a.plan(_cands(M, K, N, g), **OBJ).action
        a.step(action)
        b.step(action)
        oa, ob = _outputs(a), _outputs(b)
        for nm in oa:
            u, v = (oa[nm][:, keep], ob[nm][:, keep]) if nm == "info" else (oa[nm], ob[nm])
            assert _same(u, v), (step, nm)
    a.close()
    b.close()


# ---- 4. the refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    N = 8
    (a, stale), g = _twins(N, history=6)
    cand = _cands(2, 3, N, g)
    planners = (lambda e: e.plan(cand), lambda e: e.plan_cem(3, 1, 2, 1), lambda e: e.plan_cem_groups(2, 3, 1, 1))
    kept = dict(ALL("persistence"), values=None)
    a.set_plan_forecast(**ALL("persistence"))
    # a bad mode, by code and by name: the forecast set before stays in force
    for bad in (4, -1):
        refused(a, r"mode\[1\] = %d outside \[0, 3\]" % bad, lambda: a.set_plan_forecast(carbon=bad))
    refused(a, "not a forecast mode", lambda: a.set_plan_forecast(carbon="tomorrow"))
    s = L.SdcPlanForecast()
    s.values_entries = -1
    assert a.lib.sdc_set_plan_forecast(a._h, C.byref(s)) == -2 and b"values_entries = -1 is negative" in a.lib.sdc_last_error()
    assert a.plan_forecast == kept
    # forecast_traces with too many entries: the Python surface, and the library itself
    left = a.steps_to_episode_end()
    refused(a, "past the end of an episode", lambda: a.forecast_traces(left + 3))
    refused(a, "outside", lambda: a.forecast_traces(L.MARK_MAX_STEPS + 3))
    refused(a, "outside", lambda: a.future_traces(0))
    out = torch.empty((left + 3, N, 4), dtype=torch.float64, device=a.device)
    for n, words in ((left + 3, b"past the end of an episode"), (0, b"outside [1, 258]"), (259, b"outside [1, 258]")):
        assert a.lib.sdc_forecast_traces(a._h, n, 0, C.c_void_p(out.data_ptr()), None) == -2 and words in a.lib.sdc_last_error(), n
    assert a.lib.sdc_forecast_traces(a._h, 3, 0, None, None) == -2 and b"null out" in a.lib.sdc_last_error()
    fresh = _mk(N, ep=EP, reset=False)
    fresh.set_plan_forecast(**ALL("daily"))
    assert fresh.lib.sdc_forecast_traces(fresh._h, 3, 0, C.c_void_p(out.data_ptr()), None) == -2
    assert b"sdc_reset must be called first" in fresh.lib.sdc_last_error()
    fresh.close()
    # VALUES without values, and with too few entries (K + 2 = 5 are needed)
    short = torch.zeros((4, N, 4), dtype=torch.float64, device=a.device)
    for plan in planners:
        a.set_plan_forecast(wet_bulb="values")
        refused(a, "SDC_FORECAST_VALUES and values is null", lambda: plan(a))
        a.set_plan_forecast(wet_bulb="values", values=short)
        refused(a, "hold 4 entries, 5 are needed", lambda: plan(a))
    refused(a, "hold 4 entries, 5 are needed", lambda: a.forecast_traces(5))
    assert _same(a.forecast_traces(4)[..., 3], short[..., 3])
    refused(a, r"values must be a contiguous float64 CUDA tensor of shape \(J, n_envs, 4\)",
            lambda: a.set_plan_forecast(wet_bulb="values", values=short[:, :, :3]))
    # stale rows after a set_state write: refused while a forecast is set, planned without
    stale.set_state("t_win", stale.get_state("t_win"))
    for plan in planners[:2]:
        plan(stale)
    stale.set_plan_forecast(**ALL("persistence"))
    for plan in planners:
        refused(stale, "feature rows are not valid", lambda: plan(stale))
    a.close()
    stale.close()


# ---- 5. cleared means absent ---------------------------------------------------------------------------------------------------------
def test_cleared_and_all_perfect_mean_absent_and_deepcopy_carries_the_forecast():
    import torch
    N, M, K = 130, 3, 5
    (a, never), g = _twins(N)
    cand = _cands(M, K, N, g)
    want = never.plan(cand, **OBJ)
    assert a.plan_forecast == dict(ALL("perfect"), values=None)
    a.set_plan_forecast(**ALL("persistence"))
    assert a.plan_forecast == dict(ALL("persistence"), values=None)
    assert not _same(a.plan(cand, **OBJ).score, want.score)
    for clear in (lambda: a.set_plan_forecast(None), lambda: a.set_plan_forecast(**ALL("perfect")), lambda: a.set_plan_forecast(0, 0, 0, 0)):
        a.set_plan_forecast(**ALL("daily"))
        clear()
        assert a.plan_forecast == dict(ALL("perfect"), values=None)
        r = a.plan(cand, **OBJ)
        for nm in ("score", "returns", "best", "action"):
            assert _same(getattr(r, nm), getattr(want, nm)), nm
        assert _same(a.forecast_traces(K + 2), a.future_traces(K + 2))
    a.close()
    never.close()
    # the vector env, and copy.deepcopy of it: the modes, and `values` cloned
    n = 16
    args = {"location": "ny", "month": 6, "days_per_episode": 1, "partial_obs": True, "nonoverlapping_shared_obs_space": True}
    v = SustainDCVecEnv(args, n_envs=n, seed=3, months=[6] * n, return_torch=True)
    v.reset()
    rng = np.random.default_rng(2)
    for _ in range(5):
        v.step(torch.as_tensor(rng.integers(0, 3, (n, 3)).astype(np.int32), device=v.engine.device))
    values = _noisy(v.future_traces(K + 2), torch.Generator(device="cpu").manual_seed(1))
    v.set_plan_forecast(workload="persistence", carbon="values", wet_bulb="daily", values=values)
    cand = torch.as_tensor(rng.integers(0, 3, (M, K, n, 3)).astype(np.int32), device=v.engine.device)
    cp = copy.deepcopy(v)
    fv, fc = v.plan_forecast, cp.plan_forecast
    assert fv["values"] is values and fc["values"] is not values and fc["values"].data_ptr() != values.data_ptr()
    assert torch.equal(fc["values"], values) and {k: x for k, x in fc.items() if k != "values"} == {k: x for k, x in fv.items() if k != "values"}
    assert fv["carbon"] == "values" and fv["temperature"] == "perfect"
    rv, rc = v.plan(cand, **OBJ), cp.plan(cand, **OBJ)
    v.set_plan_forecast(None)
    oracle = v.plan(cand, **OBJ)
    for nm in ("score", "returns", "best", "action"):
        assert _same(getattr(rv, nm), getattr(rc, nm)), nm
    assert not _same(rv.score, oracle.score) and cp.plan_forecast["carbon"] == "values"      # (the copy's forecast is its own)
    v.close()
    cp.close()
