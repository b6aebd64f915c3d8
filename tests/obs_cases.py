"""Constructed traces for the observation feature rows, shared by tests/test_obs_ref.py (no GPU: the reference is finite on them and
each one still shows what it was built to show) and tests/test_gpu_obs_features.py (both device paths against the reference).

One location.  The carbon-intensity table C is a year table: the synthetic table with each case's pattern written over the days the
case owns; the workload table W is the synthetic one.  The temperature and wet-bulb windows travel per env, with the start and the
normalisation bounds, through the reset override of kind "windows" (dc_rl_amd/_args.py RESET_OVERRIDES).

A pattern is a function of k = table index - episode start, k in [-16, length): what a case computes does not move with its start
hour or with the episode length (a shorter episode sees a prefix).  Only the cases whose point IS the start (the empty past, the
hour wrap, the year-end fence) are functions of the table index itself.

A case: dict(name, day, hour, c0, ci_min, ci_max, t_min, t_max, lo, C, T, WB) -- C, T, WB[j] hold table index lo + j.
"""
import functools

import numpy as np

from dc_rl_amd import traces
from tests import obs_ref

TL = traces.TABLE_LEN
CENSUS_T = 130                  # the episode length the censuses are declared for: 131 rows deal as 64 + 64 + 3 + 0 over four wavefronts
# episode lengths on both sides of every launch shape of the features kernel (csrc/sdc_setup.hpp sdc_geometry; tests/test_obs_ref.py
# holds these to the header): 4 wavefronts | 1 wavefront | 1 wavefront without the moving averages in LDS | no rows at all
SHAPE_EDGES = {1301: (4, 1, 1), 1302: (1, 1, 1), 2357: (1, 1, 1), 2358: (1, 0, 1), 3178: (1, 0, 1), 3179: (None, None, 0)}
FULL_LDS = (1301, 2357)         # ... and the two lengths whose launch asks for exactly 65 536 bytes of LDS
SHAPE_LENGTHS = (1, 63, 64, 255, 256) + tuple(sorted(SHAPE_EDGES))
T_MAX = max(SHAPE_LENGTHS)
FIRST_DAY = 121                 # the cases lie from May on: the synthetic temperatures of the control case are not clipped at 0 there


@functools.lru_cache(maxsize=None)
def base_tables():
    """(read only: every user copies what it changes)"""
    tb = traces.synthetic_tables("ny", 0)
    for a in tb.values():
        a.setflags(write=False)
    return tb


def span_days(T):
    """days a case owns: any start hour, 16 past samples, the episode and its look-ahead"""
    return -(-(92 + T + 18 + 16) // 96)


def fence_start(T):
    """the largest whole-hour start with start + T + 17 <= TL - 1 (csrc/sdc_reset.hip: beyond it a reset raises SDC_FAULT_TABLE_RANGE)"""
    return (TL - 1 - 17 - T) // 4 * 4


def ulp(x):
    return float(np.spacing(np.float64(x)))


def triangle(k, period):
    """a triangle wave in [-1, 1] with its maximum at k = 0"""
    x = np.mod(np.asarray(k, dtype=np.float64), period) / period
    return 4.0 * np.abs(x - 0.5) - 1.0


# ---- patterns: k -> values (k a NumPy integer array; k = 0 is the episode's start) -------------------------------------------------------
def t_clipped(k, top):
    """a 0.625 K / step triangle clipped to [0, 45] (utils/managers.py:605): flat at 45 for k in [0, 48], at 0 for k in [120, 168], period 240
    (top = False: the same, starting on the flat at 0)"""
    tri = triangle(k - 24 + (0 if top else 120), 240)
    return np.clip(22.5 + 37.5 * tri, 0.0, 45.0)


def plateaus(k, up, flat, lo, step):
    """up `up` steps, flat `flat` samples, down `up` steps, flat `flat` samples, ...: every plateau is entered and left inside a window"""
    period = 2 * (up + flat)
    j = np.mod(k + 16, period)
    level = np.where(j < up, j, np.where(j < up + flat, up, np.where(j < 2 * up + flat, 2 * up + flat - j, 0)))
    return lo + step * level.astype(np.float64)


def staircase(k, seed, lo, step):
    """hourly-constant values, four equal samples each, levels from a seeded draw (the same for every length: a prefix stays a prefix)"""
    levels = np.random.default_rng(seed).integers(0, 12, size=(T_MAX + 64) // 4 + 8)
    return lo + step * levels[(k + 16) // 4].astype(np.float64)


def sawtooth(k, mid, amp, phase):
    return mid + amp * np.where((k + phase) % 2 == 0, 1.0, -1.0)


def ulp_steps(k, x):
    """x + m ulp(x), m in {0, 1, 2}"""
    m = ((k + 16) * (k + 17) // 2 + (k + 16) // 5) % 3
    return x + m.astype(np.float64) * ulp(x)


def smooth_c(idx):
    return 250.0 + 60.0 * np.sin(idx / 7.0) + 25.0 * np.sin(idx / 2.3 + 1.0)


def smooth_t(idx):
    return 21.0 + 9.0 * np.sin(idx / 11.0 + 0.5) + 2.0 * np.sin(idx / 3.1)


# name -> (what to build, the census it must show at CENSUS_T: {count: minimum rows}).  A recipe gives C and T as k -> values
# ("k"), as table index -> values ("idx"), or None: the synthetic tables where the case lies; bounds None: the 30-day min / max there.
def _recipes():
    rows = CENSUS_T + 1
    R = {}
    R["control"] = dict(hour=5, C=None, T=None, bounds=None, census={})
    R["t_flat45"] = dict(hour=2, C=None, T=("k", lambda k: t_clipped(k, True)), bounds=(None, (7.3, 48.1)), census=dict(t_sd0=30, sd0=30))
    R["t_flat0"] = dict(hour=9, C=None, T=("k", lambda k: t_clipped(k, False)), bounds=(None, (-3.7, 41.9)), census=dict(t_sd0=30, sd0=30))
    R["t_plateaus"] = dict(hour=14, C=("k", lambda k: plateaus(k, 3, 2, 210.0, 8.0)), T=("k", lambda k: plateaus(k, 5, 6, 12.0, 0.5)),
                           bounds=((190.3, 305.9), (3.1, 39.7)), census=dict(t_tie=60, ci_tie=60, tie=100))
    R["ci_staircase"] = dict(hour=7, C=("k", lambda k: staircase(k, 11, 190.0, 9.0)), T=None, bounds=((181.7, 322.3), None),
                             census=dict(ci_tie=60))
    R["ramp_up"] = dict(hour=11, C=("k", lambda k: 200.0 + 0.37 * k), T=("k", lambda k: 35.0 - 0.11 * k), bounds=((180.0, 330.0), (0.0, 45.0)),
                        census=dict(ci_none=rows, t_none=rows, none=rows))
    R["ramp_down"] = dict(hour=19, C=("k", lambda k: 300.0 * 0.997 ** k), T=("k", lambda k: 12.0 * 1.006 ** k), bounds=((150.1, 333.3), (1.7, 43.9)),
                          census=dict(ci_none=rows, t_none=rows, none=rows))
    R["saw_phase0"] = dict(hour=4, C=("k", lambda k: sawtooth(k, 240.0, 20.0, 0)), T=("k", lambda k: sawtooth(k, 20.0, 1.0, 1)),
                           bounds=((200.3, 290.9), (11.1, 33.3)), census=dict(ci_tie=rows, t_tie=rows))
    R["saw_phase1"] = dict(hour=16, C=("k", lambda k: sawtooth(k, 240.0, 20.0, 1)), T=("k", lambda k: sawtooth(k, 20.0, 1.0, 0)),
                           bounds=((200.3, 290.9), (11.1, 33.3)), census=dict(ci_tie=rows, t_tie=rows))
    # NC = C and NT = T / 32 exactly: the values ARE 0.5 + m ulp
    R["ulp_steps"] = dict(hour=21, C=("k", lambda k: ulp_steps(k, 0.5)), T=("k", lambda k: ulp_steps(k + 1, 16.0)), bounds=((0.0, 1.0), (0.0, 32.0)),
                          census=dict(ulp=rows))
    R["ulp_flat"] = dict(hour=13, C=("k", lambda k: np.full(len(k), 0.5 + ulp(0.5))), T=("k", lambda k: np.full(len(k), 16.0 + 2 * ulp(16.0))),
                         bounds=((0.0, 1.0), (0.0, 32.0)), census=dict(ci_sd0=rows, t_sd0=rows, none=rows))
    R["out_of_range"] = dict(hour=8, C=("k", lambda k: 240.0 + 70.0 * np.sin(k / 9.0)), T=("k", lambda k: 20.0 + 12.0 * np.sin(k / 13.0 + 1.0)),
                             bounds=((220.0, 260.0), (14.0, 26.0)), census=dict(nc_below=20, nc_above=20, nt_below=20, nt_above=20))
    R["hour23"] = dict(hour=23, fixed_hour=True, C=None, T=("idx", smooth_t), bounds=(None, (5.0, 37.0)), census=dict(wrapped=rows - 4))
    for c0 in (0, 4, 12):      # rows take the empty-past branch first, then the 14-point branch
        R[f"start{c0}"] = dict(day=0, hour=c0 // 4, fixed_hour=True, C=("idx", smooth_c), T=("idx", smooth_t), bounds=((150.0, 350.0), (5.0, 37.0)),
                               census=dict(no_past=16 - c0, with_past=rows - (16 - c0)))
    # (bounds of its own: the 30-day window is cut short by the year's end, by how much depends on the start)
    R["fence"] = dict(fence=True, fixed_hour=True, C=None, T=("idx", smooth_t), bounds=((171.3, 352.9), (5.0, 37.0)), census=dict(at_fence=1))
    return R


RECIPES = _recipes()
NAMES = tuple(RECIPES)
SHAPE_CASES = ("control", "t_flat45", "ci_staircase", "fence")      # the batch of the launch-shape test


def make(name, T, day=None, hour=None, length=None):
    """the case `name` for episodes of T steps starting at (day, hour); arrays for episodes up to `length` steps (default T), so that one
    set of arrays serves every shorter episode from the same start"""
    r = RECIPES[name]
    tb = base_tables()
    if r.get("fence"):
        c0 = fence_start(T)
        day, hour = c0 // 96, (c0 % 96) // 4
        lo, hi = fence_start(T_MAX if length is None else length) - 16, TL
    else:
        day = r.get("day", day)
        hour = r["hour"] if hour is None or r.get("fixed_hour") else hour
        c0 = day * 96 + hour * 4
        lo, hi = max(0, c0 - 16), c0 + (T if length is None else length) + 18
    idx = np.arange(lo, hi)
    arrays = {}
    for key, base in (("C", tb["C"]), ("T", np.clip(tb["T"], 0.0, 45.0))):
        spec = r[key]
        arrays[key] = base[lo:hi].copy() if spec is None else np.asarray(spec[1](idx - c0 if spec[0] == "k" else idx), dtype=np.float64)
    bounds = r["bounds"] or (None, None)
    ci = bounds[0] or (float(tb["C"][c0:c0 + 2880].min()), float(tb["C"][c0:c0 + 2880].max()))
    t = bounds[1] or (float(np.clip(tb["T"][c0:c0 + 2880], 0, 45).min()), float(np.clip(tb["T"][c0:c0 + 2880], 0, 45).max()))
    assert ci[1] > ci[0] and t[1] > t[0]
    return dict(name=name, day=int(day), hour=int(hour), c0=int(c0), ci_min=ci[0], ci_max=ci[1], t_min=t[0], t_max=t[1], lo=int(lo),
                C=arrays["C"], T=arrays["T"], WB=np.clip(arrays["T"] - 4.0, 0.0, 45.0), census=r["census"])


def batch(names, T, n_envs, length=None):
    """n_envs cases for one engine: `names` tiled over the batch, every env on days of its own (the cases at fixed table positions
    excepted: their copies share one pattern), the start hour moved by 7 from one round of the tiling to the next"""
    span = span_days(T if length is None else length)
    cases = []
    for e in range(n_envs):
        name = names[e % len(names)]
        cases.append(make(name, T, day=FIRST_DAY + span * e, hour=(RECIPES[name].get("hour", 0) + 7 * (e // len(names))) % 24, length=length))
    last = max(c["lo"] + len(c["C"]) for c in cases if not RECIPES[c["name"]].get("fence"))
    assert last <= fence_start(T_MAX) - 16, "the cases' days run into the year-end fence"
    return cases


def tables(cases):
    """(W, C, T, WB) year tables for an engine running `cases`: the synthetic tables with every case's carbon-intensity pattern in place"""
    tb = base_tables()
    C = tb["C"].copy()
    owner = np.full(TL, -1)
    for i, c in enumerate(cases):
        sl = slice(c["lo"], c["lo"] + len(c["C"]))
        clash = (owner[sl] >= 0) & (C[sl] != c["C"])
        assert not clash.any(), (c["name"], "writes over", cases[int(owner[sl][clash][0])]["name"])
        C[sl] = c["C"]
        owner[sl] = i
    return tb["W"], C, tb["T"], tb["WB"]


def override(cases, T):
    """the reset override of kind "windows" for an engine of len(cases) envs and episodes of T steps"""
    lw = T + 18
    win = lambda key: np.stack([c[key][c["c0"] - c["lo"]:c["c0"] - c["lo"] + lw] for c in cases])
    ov = {k: np.array([c[k] for c in cases], dtype=np.int32 if k in ("day", "hour") else np.float64)
          for k in ("day", "hour", "ci_min", "ci_max", "t_min", "t_max")}
    ov["t_win"], ov["wb_win"] = win("T"), win("WB")
    assert ov["t_win"].shape == (len(cases), lw)
    assert (ov["day"] * 96 + ov["hour"] * 4 + T + 17 <= TL - 1).all()
    return ov


def normalised(case, W):
    """(NC, NT, W, win_lo) as tests/obs_ref.trace_obs takes them: utils/managers.py:437, 608 on the case's own arrays"""
    NC = (case["C"] - case["ci_min"]) / (case["ci_max"] - case["ci_min"])
    NT = (case["T"] - case["t_min"]) / (case["t_max"] - case["t_min"])
    return NC, NT, W[case["lo"]:case["lo"] + len(NC)], case["lo"]


def reference(case, W, T, rows=None):
    """the reference on the case's rows (default: all T + 1 observations of an episode) -> (values [rows, 44] in the order of
    sorted(obs_ref.INDEX), slope scales [rows, 3], the per-row quantities)"""
    NC, NT, Wc, lo = normalised(case, W)
    rows = range(T + 1) if rows is None else rows
    cols = sorted(obs_ref.INDEX)
    val, scale, qs = np.zeros((len(rows), 44)), np.zeros((len(rows), 3)), []
    for r, s in enumerate(rows):
        q = obs_ref.trace_quantities(NC, NT, Wc, lo, case["c0"] + s, obs_ref.hour_at(case["hour"], s))
        val[r] = [q[obs_ref.INDEX[i]] for i in cols]
        scale[r] = [obs_ref.slope_scale(q["_y"][name]) for name in obs_ref.SLOPES]
        qs.append(q)
    return val, scale, qs


def _tie(g):
    """the first peak or the first valley of the gradient g is decided by a tie at zero: g > 0 then exactly 0, or g < 0 then exactly 0"""
    peaks = np.nonzero((g[:-1] > 0) & (g[1:] <= 0))[0]
    valleys = np.nonzero((g[:-1] < 0) & (g[1:] >= 0))[0]
    return bool((len(peaks) and g[peaks[0] + 1] == 0) or (len(valleys) and g[valleys[0] + 1] == 0))


def _none(g):
    return not ((g[:-1] > 0) & (g[1:] <= 0)).any() and not ((g[:-1] < 0) & (g[1:] >= 0)).any()


def census(case, qs, T):
    """how many of the case's rows show each thing a case can be for (qs: reference()'s per-row quantities, rows 0 .. T)"""
    n = dict.fromkeys(("ci_sd0", "t_sd0", "sd0", "ci_tie", "t_tie", "tie", "ci_none", "t_none", "none", "no_past", "with_past", "wrapped", "ulp",
                       "nc_below", "nc_above", "nt_below", "nt_above", "at_fence"), 0)
    for s, q in enumerate(qs):
        ci_sd0, t_sd0 = q["ci_std"] == 0, q["t_std"] == 0
        ci_tie, t_tie = _tie(q["_g"]["ci"]), _tie(q["_g"]["t"])
        ci_none, t_none = _none(q["_g"]["ci"]), _none(q["_g"]["t"])
        y = q["_y"]["t_slope"]
        flags = dict(ci_sd0=ci_sd0, t_sd0=t_sd0, sd0=ci_sd0 or t_sd0, ci_tie=ci_tie, t_tie=t_tie, tie=ci_tie or t_tie, ci_none=ci_none, t_none=t_none,
                     none=ci_none and t_none, no_past=case["c0"] + s < 16, with_past=case["c0"] + s >= 16, wrapped=case["hour"] * 4 + s >= 96,
                     ulp=0 < np.ptp(y) <= 2 * ulp(np.min(y)), nc_below=q["nc"] < 0, nc_above=q["nc"] > 1, nt_below=q["nt"] < 0, nt_above=q["nt"] > 1,
                     at_fence=s == T and case["c0"] == fence_start(T) and case["c0"] + 4 + T + 17 > TL - 1)
        for k, v in flags.items():
            n[k] += bool(v)
    return n


# ---- the launch-shape batch: SHAPE_CASES at every length of SHAPE_LENGTHS ---------------------------------------------------------------------
def shape_cases(T):
    """the four envs of the launch-shape test for episodes of T steps: the first three start where they start at every length (arrays
    for T_MAX steps: a shorter episode reads a prefix), the fence case where T puts the fence, over one pattern of the table index"""
    return batch(SHAPE_CASES, T, len(SHAPE_CASES), length=T_MAX)


@functools.lru_cache(maxsize=None)
def shape_reference():
    """the reference for the launch-shape batch, computed once: {name: (first table cursor, values, slope scales, quantities)} over
    every cursor any length reaches"""
    W = base_tables()["W"]
    out = {}
    for c in shape_cases(T_MAX):
        rows = range(TL - 18 - c["c0"] + 1) if c["name"] == "fence" else range(T_MAX + 1)
        out[c["name"]] = (c["c0"],) + reference(c, W, T_MAX, rows)
    return out


def shape_rows(case, T):
    """(values [T + 1, 44], slope scales [T + 1, 3], quantities) of `case` (one of shape_cases(T)) from shape_reference()"""
    c0, val, scale, qs = shape_reference()[case["name"]]
    a = case["c0"] - c0
    assert 0 <= a and a + T + 1 <= len(val)
    return val[a:a + T + 1], scale[a:a + T + 1], qs[a:a + T + 1]
