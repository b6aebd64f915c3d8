"""The NumPy reference of the trace-only observation entries (tests/obs_ref.py) and its constructed inputs (tests/obs_cases.py),
without a GPU:
  * the reference against the reference implementation's own recorded float32 observations in tests/golden/: bit for bit;
  * every constructed case: the reference is finite on it, and the case still shows what it was built to show (its census);
  * the constant of the slope bound, re-measured: np.polyfit against a closed form in np.longdouble;
  * the features kernel's launch shapes at the episode lengths tests/test_gpu_obs_features.py launches them at, from the header
    itself (the g++ harness of tests/test_host_setup.py).
"""
import math
import os

import numpy as np
import pytest

from tests import gpu_helpers as G          # (load_fixture only: nothing here touches a GPU)
from tests import obs_cases as K
from tests import obs_ref as R
from tests.conftest import GOLDEN_DIR
from tests.test_host_setup import ask, drivers, geometry      # noqa: F401  (the fixtures of the g++ harness)

COLS = sorted(R.INDEX)
LONG_STRIDE = 13


def fixtures_with_traces():
    every = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.endswith(".npz"))
    names = [n for n in every if {"ep0_obs", "ep0_NC"} <= set(G.load_fixture(n).files)]
    assert len(names) >= 16
    return names


def test_reference_equals_the_recorded_observations_bit_for_bit():
    """reset observation + step observations, all 44 entries, every step of the fixtures of up to 700 steps, every 13th of the longer"""
    compared = mismatches = 0
    for name in fixtures_with_traces():
        d = G.load_fixture(name)
        steps = int(d["meta_steps"])
        stride = 1 if steps <= 700 else LONG_STRIDE
        for ep in range(int(d["meta_episodes"])):
            pre = f"ep{ep}_"
            rows = [0] + [t + 1 for t in range(0, steps, stride)]        # row s: the observation at cursor0 + s
            ref, _ = R.episode_table(d[pre + "NC"], d[pre + "NT"], d[pre + "W"], int(d[pre + "win_lo"]), int(d[pre + "cursor0"]),
                                     int(d[pre + "init_hour"]), rows)
            rec = np.vstack([d[pre + "reset_obs"][None], d[pre + "obs"][::stride]])[:, COLS]
            assert rec.dtype == np.float32 and rec.shape == ref.shape
            bad = np.float32(ref) != rec
            compared += bad.size
            mismatches += int(bad.sum())
            assert not bad.any(), (name, ep, "first at (row, entry)", [(int(r), COLS[int(j)]) for r, j in np.argwhere(bad)[:5]])
    print(f"fixture values compared: {compared}, mismatches: {mismatches}")
    assert compared >= 500000 and mismatches == 0


@pytest.fixture(scope="module")
def constructed():
    """every case the GPU tests run, with its reference: the census batch (all cases over 64 envs at CENSUS_T, start hours varied)
    and the launch-shape batch at every cursor any length reaches -> [(case, T, values, slope scales, quantities)]"""
    cases = K.batch(K.NAMES, K.CENSUS_T, 64)
    W = K.tables(cases)[0]
    out = [(c, K.CENSUS_T) + K.reference(c, W, K.CENSUS_T) for c in cases]
    K.tables(K.shape_cases(K.T_MAX))
    ref = K.shape_reference()
    out += [(c, K.T_MAX) + ref[c["name"]][1:] for c in K.shape_cases(K.T_MAX)]
    return out


def test_constructed_cases_are_finite_and_show_what_they_are_for(constructed):
    seen = set()
    for case, T, val, scale, qs in constructed:
        assert np.isfinite(val).all() and np.isfinite(scale).all(), case["name"]
        nc_nt = np.array([[q["nc"], q["nt"]] for q in qs])
        assert np.abs(nc_nt).max() <= 2.5, (case["name"], np.abs(nc_nt).max())        # |NC|, |NT| at or below about 2
        if T != K.CENSUS_T or case["name"] in seen:
            continue
        seen.add(case["name"])
        got = K.census(case, qs, T)
        print(case["name"], "day", case["day"], "hour", case["hour"], {k: v for k, v in got.items() if v})
        for what, least in case["census"].items():
            assert got[what] >= least, (case["name"], what, got[what], "of", T + 1, "rows; declared", least)
    assert seen == set(K.NAMES)
    # the control case is ordinary data: none of the degenerate rows
    control = next(K.census(c, qs, T) for c, T, _, _, qs in constructed if c["name"] == "control" and T == K.CENSUS_T)
    assert control["sd0"] == 0 and control["ulp"] == 0 and control["no_past"] == 0


def test_launch_shape_batch_keeps_its_point_at_every_length():
    """a shorter episode reads a prefix of the same windows, so the flat rows and the ties come first: even T = 1 has them"""
    for T in K.SHAPE_LENGTHS:
        cases = K.shape_cases(T)
        K.override(cases, T)
        K.tables(cases)
        by = {c["name"]: K.census(c, K.shape_rows(c, T)[2], T) for c in cases}
        assert by["t_flat45"]["t_sd0"] >= min(T + 1, 30) and by["fence"]["at_fence"] == 1, (T, by)
        assert by["ci_staircase"]["ci_tie"] >= (T + 1) // 2, (T, by["ci_staircase"])
        assert T < 200 or by["t_flat45"]["t_sd0"] >= T // 10      # (the clipped triangle comes round: flat rows all along a long episode)


def test_slope_constant_covers_numpy_polyfit(constructed):
    """SLOPE_C >= 4 x the worst |np.polyfit - longdouble closed form| / (2^-53 max|y|) over every slope window of every constructed case"""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than a double here: nothing to size the bound with"
    worst, where, n = 0.0, None, 0
    for case, T, val, scale, qs in constructed:
        for s, q in enumerate(qs):
            for name in R.SLOPES:
                y = q["_y"][name]
                m = R.slope_scale(y)
                n += 1
                if m == 0.0:
                    assert q[name] == 0.0
                    continue
                dev = float(abs(np.longdouble(q[name]) - R.slope_longdouble(y)) / (np.longdouble(2.0) ** -53 * m))
                if dev > worst:
                    worst, where = dev, (case["name"], T, s, name)
    print(f"slope windows: {n}, worst |np.polyfit - closed form| = {worst:.3f} x 2^-53 max|y| at {where}; "
          f"{R.SLOPE_SAFETY} x that, rounded up: {math.ceil(R.SLOPE_SAFETY * worst)}; SLOPE_C = {R.SLOPE_C}")
    assert R.SLOPE_C >= R.SLOPE_SAFETY * worst


def test_feature_launch_shapes_at_the_lengths_the_gpu_test_runs(ask):      # noqa: F811
    lengths = sorted(K.SHAPE_EDGES)
    for T, g in zip(lengths, geometry(ask, [(4, T, 0) for T in lengths])):
        waves, sma, has = K.SHAPE_EDGES[T]
        assert g["has_feat"] == has, T
        if has:
            assert (g["feat_waves"], g["feat_use_sma"]) == (waves, sma), (T, g)
        assert (g["feat_lds_bytes"] == 65536) == (T in K.FULL_LDS), (T, g["feat_lds_bytes"])
    # ... and these ARE the header's boundaries: the shape changes between each pair, and nowhere else up to the first length without rows
    scan = list(range(1, max(lengths) + 2))
    shape = [(g["has_feat"], g["feat_waves"] if g["has_feat"] else 0, g["feat_use_sma"] if g["has_feat"] else 0)
             for g in geometry(ask, [(4, T, 0) for T in scan])]
    changes = [T for T, a, b in zip(scan[1:], shape, shape[1:]) if a != b]
    assert changes == [1302, 2358, 3179] and set(changes) | {T - 1 for T in changes} == set(lengths)
