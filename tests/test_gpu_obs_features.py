"""The 44 trace-only observation entries on the device, from both places that compute them, against the NumPy reference of
tests/obs_ref.py on the constructed traces of tests/obs_cases.py:

  * the episode's feature rows (csrc/sdc_features.hip, one lane per episode step), which every specialised step kernel loads, and
  * the whole-wavefront path (csrc/sdc_device.hpp stage_windows / build_obs_pool): the reset observation, every step of an env whose
    rows are stale (here: after set_state("t_win") with the same values), and episodes too long for rows.

Device against reference, per entry: everything but the three least-squares slopes as fp32 bits; the slopes within
2^-24 |ref| + SLOPE_C 2^-53 max|y| (tests/obs_ref.py: the fp32 cast + np.polyfit's own distance from the exact slope, measured on
the CPU by tests/test_obs_ref.py), and as bits too on the control case.  Between the device paths: every output of every step equal,
torch.equal, the diagnostics column `reserved` masked.
"""
import numpy as np
import pytest

from dc_rl_amd import _args as A
from dc_rl_amd import _lib as L
from dc_rl_amd import dc_config
from dc_rl_amd.engine import SdcEngine
from tests import gpu_helpers as G
from tests import obs_cases as K
from tests import obs_ref as R
from tests import step_paths

pytestmark = pytest.mark.gpu

COLS = sorted(R.INDEX)
EXACT = [j for j, i in enumerate(COLS) if i in R.EXACT_INDEX]
SLOPE = [j for j, i in enumerate(COLS) if i in R.SLOPE_INDEX]
SLOPE_SCALE = [R.SLOPES.index(R.INDEX[COLS[j]]) for j in SLOPE]      # which of a row's three slope scales entry j is held to
OUTPUTS = ("obs", "share", "rew", "done", "info")


def run_episode(cases, tables, T, flags, acts, rewrite_before=None):
    """one engine, one whole episode of T steps -> ({output: device tensor [T + 1 or T, N, ...]}, the step kernels by step).  obs and
    share have the reset's as row 0.  rewrite_before: the step index before which the weather windows are written again, same values."""
    import torch
    N = len(cases)
    ov = K.override(cases, T)
    eng = SdcEngine(N, episode_steps=T, auto_reset=False, debug_flags=flags)
    try:
        eng.set_tables(0, *tables)
        eng.set_dc_params(0, dc_config.size_datacenter("dc_config.json", 1, 30.0))
        eng.assign(0, 0, 0, 364)
        obs0, share0 = (x.clone() for x in eng.reset(override=ov))
        flat = torch.empty((T, eng.out_flat.numel()), dtype=torch.uint8, device=eng.device)      # one copy per step, one fetch per episode
        kernels = []
        for t in range(T):
            if t == rewrite_before:
                eng.set_state("t_win", ov["t_win"])
            eng.step(acts[t])
            flat[t].copy_(eng.out_flat)
            kernels.append(eng.last_step_kernel())
        torch.cuda.synchronize()
    finally:
        eng.close()
    out = {}
    for name, dtype, shape, off in A.out_layout(N)[0]:
        if name == "done":
            out[name] = flat[:, off * 4:].contiguous()
        else:
            out[name] = flat[:, off * 4:(off + int(np.prod(shape))) * 4].contiguous().view(torch.float32).view((T,) + shape)
    out["obs"] = torch.cat([obs0[None], out["obs"]])
    out["share"] = torch.cat([share0[None], out["share"]])
    assert (out["info"][:, :, L.INFO_IDX["fault"]] == 0).all(), "a constructed case raised info[fault]"
    assert int(out["done"][:-1].sum()) == 0 and int(out["done"][-1].sum()) == N
    return out, kernels


def actions(T, N, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 3, (T, N, 3), dtype=torch.int32, generator=g).cuda()


def cross_path_mismatches(a, b):
    """outputs of two engines that must agree to the bit -> the number of values that differ (asserted 0 by the caller through torch.equal)"""
    import torch
    n = 0
    for name in OUTPUTS:
        u, v = a[name], b[name]
        if name == "info":       # (the diagnostics column says HOW the reward state was served, which a host write may change)
            u, v = u.clone(), v.clone()
            u[..., L.INFO_IDX["reserved"]] = 0
            v[..., L.INFO_IDX["reserved"]] = 0
        differ = int((u != v).sum())
        assert torch.equal(u, v), (name, "values that differ:", differ, "first at (step, env, ...)", (u != v).nonzero()[0].tolist())
        n += differ
    return n


def against_reference(out, cases, rows_of):
    """every observation of an episode (the reset's and each step's) against NumPy -> (values compared, worst slope error / its bound)"""
    raw = G.raw_obs(out["obs"].cpu().numpy())                  # [T + 1, N, 53] float32
    compared, worst = 0, 0.0
    for e, case in enumerate(cases):
        val, scale, _ = rows_of(case)
        dev = raw[:, e][:, COLS]
        assert dev.shape == val.shape and dev.dtype == np.float32
        bad = dev[:, EXACT] != np.float32(val[:, EXACT])
        assert not bad.any(), (case["name"], "env", e, int(bad.sum()), "entries differ from the reference; first (row, raw-obs entry, device, reference):",
                               [(int(r), COLS[EXACT[int(j)]], float(dev[r, EXACT[j]]), float(val[r, EXACT[j]])) for r, j in np.argwhere(bad)[:4]])
        ref = val[:, SLOPE]
        err = np.abs(dev[:, SLOPE].astype(np.float64) - ref)
        bound = 2.0 ** -24 * np.abs(ref) + R.SLOPE_C * 2.0 ** -53 * scale[:, SLOPE_SCALE]
        ratio = np.where(err > 0, err / np.where(bound > 0, bound, 1.0), 0.0)        # (a window of zeros: slope 0 on both sides, or it fails)
        ratio = np.where((bound == 0) & (err > 0), np.inf, ratio)
        worst = max(worst, float(ratio.max()))
        assert (err <= bound).all(), (case["name"], "env", e, "slope beyond its bound; first (row, raw-obs entry, device, reference, error / bound):",
                                      [(int(r), COLS[SLOPE[int(j)]], float(dev[r, SLOPE[j]]), float(ref[r, j]), float(ratio[r, j]))
                                       for r, j in np.argwhere(err > bound)[:4]])
        if case["name"] == "control":
            same = dev[:, SLOPE] == np.float32(ref)
            assert same.all(), ("control: slopes not bit-equal to np.polyfit after the cast", int((~same).sum()))
        compared += dev.size
    return compared, worst


# ---- A: constructed traces on every consumer of the rows ----------------------------------------------------------------------------------
MAPPINGS = {"general": step_paths.GENERAL, "pair": step_paths.PAIR, "quad": step_paths.QUAD, "wide": step_paths.WIDE}
REWRITE_AFTER = 37


@pytest.fixture(scope="module")
def census_batch():
    """all cases tiled over 64 envs, start hours varied; T = 130: 131 rows deal as 64 + 64 + 3 + 0 over the four wavefronts"""
    T, N = K.CENSUS_T, 64
    cases = K.batch(K.NAMES, T, N)
    tables = K.tables(cases)
    refs = [K.reference(c, tables[0], T) for c in cases]
    return T, cases, tables, {id(c): r for c, r in zip(cases, refs)}, actions(T, N, 130)


@pytest.mark.parametrize("mapping", sorted(MAPPINGS))
def test_constructed_traces_on_every_consumer_of_the_rows(census_batch, mapping):
    T, cases, tables, refs, acts = census_batch
    general, own = step_paths.KERNEL_NAME["general"], step_paths.KERNEL_NAME[mapping]
    rows, k_rows = run_episode(cases, tables, T, MAPPINGS[mapping], acts)                                      # keeps its rows
    stale, k_stale = run_episode(cases, tables, T, MAPPINGS[mapping], acts, rewrite_before=0)                  # computes every step
    late, k_late = run_episode(cases, tables, T, MAPPINGS[mapping], acts, rewrite_before=REWRITE_AFTER)        # rows, then computes
    assert set(k_rows) == {own} and set(k_stale) == {general}      # (stale rows: the general kernel, which then computes the features itself)
    assert set(k_late[:REWRITE_AFTER]) == {own} and set(k_late[REWRITE_AFTER:]) == {general}
    compared, worst = against_reference(rows, cases, lambda c: refs[id(c)])
    differ = cross_path_mismatches(rows, stale) + cross_path_mismatches(rows, late)
    print(f"obs features, T = {T}, {mapping} ({own}): {compared} values against NumPy, worst slope error {worst:.3f} of its bound, "
          f"cross-path mismatches over 2 x {T} steps of {len(cases)} envs: {differ}")
    assert differ == 0


# ---- B: every launch shape of the features kernel ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_tables():
    return K.tables(K.shape_cases(K.T_MAX))       # (the same year tables at every length: the fence case writes nothing into them)


@pytest.mark.parametrize("T", K.SHAPE_LENGTHS)
def test_every_launch_shape_of_the_features_kernel(shape_tables, T):
    """4 wavefronts with the moving averages in LDS up to T = 1301 (65 536 bytes of LDS exactly there), one wavefront up to 2357 (65 536
    bytes again), one without the moving averages up to 3178, no rows from 3179: whole episodes of the control case, a temperature
    window clipped flat and then leaving, a carbon-intensity staircase and the start at the year-end fence"""
    cases = K.shape_cases(T)
    acts = actions(T, len(cases), T)
    rows, kernels = run_episode(cases, shape_tables, T, 0, acts)
    has_rows = K.SHAPE_EDGES.get(T, (4, 1, 1))[2]
    assert set(kernels) == {step_paths.KERNEL_NAME["pair" if has_rows else "general"]}
    compared, worst = against_reference(rows, cases, lambda c: K.shape_rows(c, T)[:2] + (None,))
    differ = None
    if T in K.SHAPE_EDGES and has_rows:
        stale, k_stale = run_episode(cases, shape_tables, T, 0, acts, rewrite_before=0)
        assert set(k_stale) == {step_paths.KERNEL_NAME["general"]}
        differ = cross_path_mismatches(rows, stale)
        assert differ == 0
    print(f"obs features, T = {T}, {kernels[0]}: {compared} values against NumPy, worst slope error {worst:.3f} of its bound, "
          f"cross-path mismatches: {differ}")
