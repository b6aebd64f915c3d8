"""The history-normalised reward's device code (dc_rl_amd/csrc/sdc_trackers.hpp, sdc_halfwin.hpp, sdc_quadwin.hpp, sdc_ringpath.hpp),
function by function on the device, through tests/aux/reward_probe.hip -- a test-only translation unit over the real headers, built with
the library's flags.  The reference is the sorted-list model of tests/reward_model.py; the inputs, what the model expects of each and
the checkers live in tests/reward_cases.py, and tests/test_reward_probe.py proves them sound on the CPU (the censuses of the branches the
inputs reach, the checkers failing on a corrupted expectation, the moment bounds met by the algorithm alone).

Measured on MI355X (each test prints its figures): wave_sum_f64 0.029 of its summation bound; the windows' crossing sums 0.032 of theirs;
rebuild_state's sums and the small histories' sd at most 0.105 of their bounds; clipped_moments 0.50 (mean), 0.27 (sd), 0.27 (1 / sd) of
its derived bounds; 23 of 256 refills list a different number of keys in the one-wavefront and the cooperative form (both valid).
clip_bounds: before these tests klb was 0x80000000 where lb == +0.0 (by definition 0x7FFFFFFF, the key of -0.0) and kub 0x80000000
where ub == -0.0 (by definition 0x80000001): klb in 903 of the 173 656 cases; fixed in sdc_trackers.hpp.

Not here: the lane-per-env window code inside the kernel body of sdc_wide.hip (tests/test_gpu_wide.py holds it to the quad kernel).
"""
import numpy as np
import pytest

from tests import reward_cases as K
from tests import reward_model as M
from tests import reward_probe as RP

pytestmark = pytest.mark.gpu
U32 = np.uint32


# ---- keys ----------------------------------------------------------------------------------------------------------------------------------------
def test_keys_round_trip_and_are_strictly_monotone():
    rng = np.random.default_rng(1)
    pows = 2.0 ** np.arange(-10, 21)
    p32 = pows.astype(np.float32)
    special = np.concatenate([p32, np.nextafter(p32, np.float32(0)), np.nextafter(p32, np.float32(np.inf)),
                              np.array([0.0, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, np.inf], dtype=np.float32)])
    with np.errstate(over="ignore"):      # (some products overflow to +-inf: duplicates of the two infinities, removed below)
        wide = rng.normal(0.0, 1.0, 100_000).astype(np.float32) * (10.0 ** rng.integers(-40, 39, 100_000)).astype(np.float32)
    v = np.concatenate([special, -special, wide])
    v = v[~np.isnan(v)]
    bits = v.view(U32)
    # the fp32 total order: by value, -0.0 before +0.0
    order = np.lexsort((~np.signbit(v), v))
    bits = bits[order]
    bits = bits[np.r_[True, bits[1:] != bits[:-1]]]
    key, back = RP.keys(bits)
    assert (back == bits).all(), "key_f32(f32_key(x)) is not x"
    assert (np.diff(key.astype(np.int64)) > 0).all(), "f32_key is not strictly monotone in the fp32 total order"
    assert (key == M.f32_key(bits)).all()
    f = bits.view(np.float32)
    assert np.isinf(f[0]) and np.isinf(f[-1]) and (f == 0).sum() == 2 and ((f != 0) & (np.abs(f) < 1.17549435e-38)).sum() >= 4
    assert (key != M.KEY_NONE).all()
    # every bit pattern class round-trips, NaNs and the empty-slot key included
    allb = np.concatenate([rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(U32), np.array([0x7FFFFFFF, 0xFFFFFFFF, 0x7FC00000], dtype=U32)])
    key, back = RP.keys(allb)
    assert (back == allb).all() and (key == M.f32_key(allb)).all() and key[-3] == M.KEY_NONE


# ---- reduce --------------------------------------------------------------------------------------------------------------------------------------
def test_wave_half_and_row_reductions():
    rng = np.random.default_rng(2)
    n = 512
    u = rng.integers(0, 1 << 32, (n, 64), dtype=np.uint64).astype(U32)
    u[0], u[1], u[2] = 0, 0xFFFFFFFF, np.arange(64)
    u[3:40] >>= rng.integers(0, 31, (37, 1)).astype(U32)
    d = rng.normal(0.0, 1.0, (n, 64)) * 10.0 ** rng.integers(-8, 9, (n, 64))
    exact = n // 2                                    # the second half: integers below 2^40, every partial sum exactly representable
    d[exact:] = rng.integers(-(1 << 40), 1 << 40, (n - exact, 64)).astype(np.float64)
    o = RP.reduce(u, d)
    s = u.astype(np.uint64)
    assert (o["wave_sum_u32"] == (s.sum(axis=1) & 0xFFFFFFFF)[:, None]).all()
    assert (o["wave_min_u32"] == u.min(axis=1)[:, None]).all() and (o["wave_max_u32"] == u.max(axis=1)[:, None]).all()
    half = (s.reshape(n, 2, 32).sum(axis=2) & 0xFFFFFFFF).repeat(32, axis=1)
    row = (s.reshape(n, 4, 16).sum(axis=2) & 0xFFFFFFFF).repeat(16, axis=1)
    assert (o["half_sum_u32"] == half).all() and (o["row_sum_u32"] == row).all()
    # fp64: the summation bound of any tree over m terms, (m - 1) eps sum |v|
    mag = np.abs(d)
    ref = np.array([M.exact_sum(r) for r in d])
    err = np.abs(o["wave_sum_f64"] - ref[:, None])
    bound = 63 * M.EPS * mag.sum(axis=1)[:, None]
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (o["wave_sum_f64"] == o["wave_sum_f64"][:, :1]).all()                        # wave-uniform
    href = np.array([[M.exact_sum(r[:32]), M.exact_sum(r[32:])] for r in d]).repeat(32, axis=1)
    rref = np.array([[M.exact_sum(r[16 * j:16 * j + 16]) for j in range(4)] for r in d]).repeat(16, axis=1)
    hb = 31 * M.EPS * mag.reshape(n, 2, 32).sum(axis=2).repeat(32, axis=1)
    rb = 15 * M.EPS * mag.reshape(n, 4, 16).sum(axis=2).repeat(16, axis=1)
    assert (np.abs(o["half_sum_f64"] - href) <= hb).all() and (np.abs(o["row_sum_f64"] - rref) <= rb).all()
    print("wave_sum_f64 worst error / bound: %.3g" % float((err[:exact] / bound[:exact]).max()))
    # "the same tree": exactly representable sums are exact in all three forms, and the forms compose bit for bit
    assert (o["wave_sum_f64"][exact:] == ref[exact:, None]).all()
    assert (o["half_sum_f64"][exact:] == href[exact:]).all() and (o["row_sum_f64"][exact:] == rref[exact:]).all()
    # on every input: a half's sum is the sum of its two rows' sums, and the wave's sum is the sum of the two halves' sums
    rs, hs = o["row_sum_f64"], o["half_sum_f64"]
    assert (hs[:, 0] == rs[:, 16] + rs[:, 0]).all() and (hs[:, 32] == rs[:, 48] + rs[:, 32]).all()
    assert (o["wave_sum_f64"][:, 0] == hs[:, 32] + hs[:, 0]).all()


# ---- window ops ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def window_runs():
    W = K.window_ops()
    return {form: RP.window_ops(form, W["keys0"], W["meta"], W["ops"], W["iv"]) for form in RP.FORMS}


@pytest.mark.parametrize("form", list(RP.FORMS))
def test_window_ops_against_the_sorted_list_model(window_runs, form):
    """After every op: the model's (r0, hi) -- so no window is dropped on a consistent sequence, and inconsistent case (a) drops it --,
    the window contract, `changed` as the rules give it and never false when a key register changed, resolve / spans / first and last
    key / crossing counts exactly, the crossing sums within 63 eps sum |term| of the exact sums; slots with `on` false untouched."""
    keys, oi, od = window_runs[form]
    fig = K.check_window_ops(form, keys, oi, od, has_on=form != "QTrack", has_spans=form != "QWin")
    W = K.window_ops()
    bad = W["bad_at"]
    for s in np.flatnonzero(bad >= 0):
        hi = oi[s, :, RP.OI["hi"]].astype(np.int64)
        assert hi[bad[s] - 1] > 0 and (hi[bad[s]:] == 0).all(), (form, int(s))
    print(f"{form}: crossing sums' worst error / bound {fig['worst_sum_ratio']:.3g}; `changed` true with the registers' bits unchanged "
          f"(an eviction and an insertion that cancel, a shift of equal keys) in {fig['over_reported']} slot-ops")


def test_the_three_window_forms_give_identical_windows(window_runs):
    W = K.window_ops()
    on = W["on"]
    cols = [RP.OI[c] for c in ("r0", "hi", "ch", "ok1", "ok3", "any0", "c0", "any1", "c1", "first", "last", "n")]
    kq, iq, dq = window_runs["QTrack"]
    for form in ("HWin", "QWin"):
        k, i, d = window_runs[form]
        assert (k[on] == kq[on]).all() and (i[on][:, :, cols] == iq[on][:, :, cols]).all(), form
    # the half-wave and the quad form reduce the crossing sums in the same tree: bit for bit
    assert (window_runs["HWin"][2][on].view(np.uint64) == window_runs["QWin"][2][on].view(np.uint64)).all()


# ---- refill ----------------------------------------------------------------------------------------------------------------------------------------
def test_refills_against_the_sorted_ring():
    R = K.refill_cases()
    runs = {w: RP.refill(w, R["ring"], R["win"], R["meta"]) for w in ("refill5", "refill10", "refill_coop")}
    fails = []
    for c in range(len(R["notes"])):
        r0s = []
        for which, (keys, om) in runs.items():
            for wv in range(keys.shape[1]):
                bad = K.check_refill(c, keys[c, wv], int(om[c, wv, 0]), int(om[c, wv, 1]), R)
                if bad:
                    fails.append((c, R["notes"][c]["feature"], which, wv, bad))
                if om[c, wv, 1] > 0:
                    # (the kept part's rank: r0 going up, the last rank going down)
                    r0s.append(int(om[c, wv, 0]) if R["meta"][c][2] == K.UP else int(om[c, wv, 0]) + int(om[c, wv, 1]))
        if R["notes"][c]["consistent"]:
            assert len(r0s) == 6 and len(set(r0s)) == 1, (c, R["notes"][c], r0s)
        k5, k10, kc = runs["refill5"][0][c, 0], runs["refill10"][0][c, 0], runs["refill_coop"][0][c]
        assert (k5 == k10).all() and (runs["refill5"][1][c] == runs["refill10"][1][c]).all(), (c, "the two batch sizes differ")
        assert (kc == kc[0]).all() and (runs["refill_coop"][1][c] == runs["refill_coop"][1][c, 0]).all(), (c, "the four wavefronts differ")
    assert not fails, (len(fails), fails[:6])
    his = {w: om[:, 0, 1] for w, (_, om) in runs.items()}
    print("refill: 256 rings; cases where the one-wavefront and the cooperative form list a different number of keys:",
          int((his["refill5"] != his["refill_coop"]).sum()))


# ---- rebuild, bisection, window builder ------------------------------------------------------------------------------------------------------------
def test_bisection_and_window_builder_against_the_sorted_ring():
    R = K.rebuild_cases()
    k4, keys, oi = RP.bisect_build(R["ring"], R["bmeta"])
    fails = [(c, R["notes"][c], bad) for c in range(len(k4)) for bad in [K.check_bisect(c, k4[c], keys[c], oi[c])] if bad]
    assert not fails, (len(fails), fails[:6])


def test_rebuild_state_against_the_sorted_ring():
    R = K.rebuild_cases()
    X = K.rebuild_expectations()
    keys, oi, od = RP.rebuild(R["ring"], R["meta"])
    fails, worst = [], 0.0
    for c in range(len(X)):
        bad, w = K.check_rebuild(c, keys[c], oi[c], od[c], X)
        worst = max(worst, w)
        if bad:
            fails.append((c, R["notes"][c], bad))
    print("rebuild_state: 128 rings; worst error / bound of a sum or a small history's sd: %.3g" % worst)
    assert not fails, (len(fails), fails[:6])


# ---- bounds and moments ------------------------------------------------------------------------------------------------------------------------------
def test_clip_bounds_against_numpys_lerp_and_the_definition_of_the_bound_keys():
    B = K.bounds_cases()
    od, ou = RP.bounds(B[0], B[1], B[2], B[3], B[4])
    K.check_bounds(od, ou, B)
    print("clip_bounds:", B.shape[1], "cases; lb / ub / ctr equal numpy's lerp (+-0 equal), klb / kub by definition")


def test_clipped_moments_against_the_exact_function_of_its_inputs():
    """mean within 4 eps (|A1| + |T1|) / n; sd and 1 / sd within 8 eps m2 / var + 1e-15 relative where var > 1e-30 and ub > lb (the
    cancellation in m2 - mean^2: 2 eps on m2, 5 eps on mean^2, both at most m2, halved by the root, plus inv_sqrt_pos' stated 3e-16 and
    the product's rounding), else sd == 0 and inv_sd == 1 exactly; eps = 2^-53.
    Measured on MI355X: worst ratio to the bound 0.50 (mean), 0.27 (sd), 0.27 (1 / sd)."""
    C = K.moments_cases()
    out = RP.moments(C["n"], C["n_full"], C["lb"], C["ub"], C["A1"], C["A2"], C["T1"], C["T2"])
    w = K.check_moments(out[0], out[1], out[2], C)
    print("clipped_moments: worst ratio to the bound: mean %.3g, sd %.3g, 1 / sd %.3g (%d cases with var > 1e-30, %d with sd == 0)"
          % (w["mean"], w["sd"], w["inv_sd"], w["n_pos"], w["n_zero"]))
