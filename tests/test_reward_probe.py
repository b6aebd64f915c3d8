"""The function-level reward tests' CPU side (tests/test_gpu_reward_functions.py is the device side): the probe cross-compiles with the
library's flags and exports every launcher; the sorted-list model's lerp is numpy's percentile; the inputs reach every branch they are
meant to reach (the censuses, printed); the checkers fail on a corrupted expectation; the derived moment bounds are met by the algorithm
alone, restated in NumPy."""
import os
import subprocess

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import physics_probe as PP
from tests import reward_cases as K
from tests import reward_model as M
from tests import reward_probe as RP


def test_probe_cross_compiles_with_the_librarys_flags_and_exports_every_launcher(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path / "libreward_probe.so")
    cmd = RP.build_command(out)
    for flag in L.HIPCC_FLAGS:
        assert flag in cmd
    assert "-ffp-contract=off" in cmd and "--offload-arch=gfx950" in cmd
    subprocess.run(cmd, check=True, cwd=RP.ROOT)
    syms = subprocess.run(["nm", "-D", "--defined-only", out], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for name in RP.LAUNCHERS:
        assert "probe_" + name in exported, name


def test_no_product_file_names_the_probe():
    for root, _, files in os.walk(os.path.dirname(os.path.abspath(L.__file__))):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".c", ".h")):
                text = open(os.path.join(root, f), errors="replace").read()
                assert "reward_probe" not in text and "probe_build" not in text, f


def test_both_probes_share_one_copy_of_the_build_logic(monkeypatch):
    from tests import probe_build
    assert type(PP._PROBE) is type(RP._PROBE) is probe_build.Probe
    assert os.path.dirname(PP.LIB_PATH) == os.path.dirname(RP.LIB_PATH) == probe_build.OUT_DIR
    assert os.path.basename(RP.LIB_PATH) == "libreward_probe.so" and os.path.basename(PP.LIB_PATH) == "libphysics_probe.so"
    # a missing library is an error that names the build command
    missing = probe_build.Probe("reward_probe", "reward probe")
    monkeypatch.setattr(missing, "lib_path", os.path.join(probe_build.OUT_DIR, "no_such_probe.so"))
    with pytest.raises(RuntimeError) as err:
        missing.load(lambda lib: None)
    assert "not built" in str(err.value) and "g.build()" in str(err.value)


def test_keys_order_values_and_round_trip():
    v = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf], dtype=np.float32)
    k = M.key_of(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()                       # -0.0 and +0.0 are adjacent distinct keys
    assert int(k[5]) - int(k[4]) == 1
    assert (M.key_bits(k) == v.view(np.uint32)).all()


def test_the_models_lerp_is_numpys_percentile():
    """The restatement clip_bounds uses (numpy's _lerp on the keys at ranks k, k + 1) equals np.percentile(h, [25, 75]) in value on
    6000 random histories, quantised ones with heavy ties included; in bits it differs only in the sign of a zero."""
    rng = np.random.default_rng(31)
    differs = 0
    for i in range(6000):
        n = int(rng.integers(2, 400))
        kind = i % 3
        v = rng.normal(0.0, 10.0, n) if kind == 0 else (np.round(rng.normal(0.0, 2.0, n)) if kind == 1 else rng.integers(-2, 3, n) * 0.5)
        v = np.asarray(v, dtype=np.float32)
        h = np.sort(M.key_of(v))
        q1, q3, _, _, _ = M.bounds_from_keys(n, *M.quartile_keys([int(x) for x in h]))
        ref = np.percentile(M.key_f64(h), [25, 75])
        got = np.array([q1, q3], dtype=np.float64)
        assert (got == ref).all(), (i, n, got, ref)
        bits = got.view(np.uint64) != ref.view(np.uint64)
        if bits.any():
            differs += int(bits.sum())
            assert (ref[bits] == 0.0).all() and (got[bits] == 0.0).all()
    print("quartiles that differ from numpy's in the sign of zero only:", differs)


def test_window_op_inputs_reach_every_outcome():
    W = K.window_ops()
    print("window-op outcome census (the slots with `on`, all three forms run the same inputs):", W["census"])
    print("spans() true on", W["spans_true"], "intervals; crossings with at least one key:", W["crossings"],
          "; slots with inconsistent case (a):", int((W["bad_at"] >= 0).sum()))
    for name in M.OUTCOMES:
        assert W["census"][name] >= 50, name
    assert W["census"]["inconsistent"] >= 4 and W["spans_true"] >= 1000 and W["crossings"] >= 1000
    assert int((~W["on"]).sum()) == K.N_OFF
    m = W["meta"]
    assert (m[:, 1] >= 0).all() and (m[:, 1] <= M.WIN).all() and (m[:, 2] == 0).sum() == K.N_EMPTY
    assert (W["exp_i"][:, :, 3].max(axis=1) > 64).any() and set(K.CAPACITIES) == {33, 64, 65, 100, 257}


def test_refill_inputs_reach_every_branch():
    C = K.refill_census()
    print("refill census:", C)
    for coop in (False, True):
        assert C["rounds2"][coop] >= 20 and C["d0"][coop] >= 20
    assert min(C["side"].values()) >= 50 and min(C["dir"].values()) >= 50 and C["reaches_end"] >= 10 and C["inconsistent"] >= 10
    assert C["dropped_consistent"] == 0
    R = K.refill_cases()
    m = R["meta"]
    assert len(m) == 256 and set(m[:, 4].tolist()) == {65, 100, 1500, 10000, 10240}
    assert m[:, 1].min() == 13 and m[:, 1].max() == 64
    assert {int(p) % 4 for p in m[:, 5] if p >= 0} == {0, 1, 2, 3}
    assert {(n["feature"], n["run_len"]) for n in R["notes"] if n["feature"] == "run"} == {("run", r) for r in (1, 4, 5, 63, 64, 300)}


def test_rebuild_inputs():
    R = K.rebuild_cases()
    assert len(R["hists"]) == 128 and {len(h) for h in R["hists"]} == set(K.REBUILD_NS)
    X = K.rebuild_expectations()
    share = [(e["qc"][0] + e["qc"][1]) / e["n"] for e in X if e["n"] >= 1500]
    print("rebuild: tail shares at n >= 1500:", sorted(round(s, 4) for s in share))
    assert min(share) == 0.0 and max(share) > 0.05
    assert any(e["lb"] == e["ub"] for e in X)                          # iqr == 0
    # the model's own windows meet the contract it states
    for c, e in enumerate(X):
        h = [int(x) for x in R["hists"][c]]
        for a, b in (e["q1"], e["q3"], e["bu"], e["bl"]):
            w = M.Window(h, a, b - a + 1)
            assert M.contract_violation(w.keys(), a, b - a + 1, h) is None


def test_the_window_checker_bites():
    ek, gi, gd = K.expected_as_output()
    K.check_window_ops("model", ek, gi, gd)
    W = K.window_ops()
    E = W["exp_i"]
    s, t = (int(x) for x in np.argwhere((E[:, :, 1] >= 2) & W["on"][:, None] & ~W["dead"] & (ek[:, :, 0] != ek[:, :, 1]))[100])
    k2 = ek.copy()
    k2[s, t, 0], k2[s, t, 1] = ek[s, t, 1], ek[s, t, 0]                # two window keys swapped
    with pytest.raises(AssertionError, match="window keys"):
        K.check_window_ops("model", k2, gi, gd)
    g2 = gi.copy()
    g2[s, t, RP.OI["r0"]] += 1                                          # r0 off by one
    with pytest.raises(AssertionError, match="r0"):
        K.check_window_ops("model", ek, g2, gd)
    s, t = (int(x) for x in np.argwhere((W["cross"][0]["c"] > 0) & W["on"][:, None] & ~W["dead"])[7])
    g2 = gi.copy()
    g2[s, t, RP.OI["c0"]] += 1                                          # one tail count off by one
    with pytest.raises(AssertionError, match="crossing count"):
        K.check_window_ops("model", ek, g2, gd)
    d2 = gd.copy()
    d2[s, t, 0] *= 1.0 + 1e-13
    if d2[s, t, 0] != gd[s, t, 0]:
        with pytest.raises(AssertionError, match="crossing sum"):
            K.check_window_ops("model", ek, gi, d2)
    g2 = gi.copy()
    g2[s, t, RP.OI["hi"]] = 0                                           # a wrongly dropped window
    with pytest.raises(AssertionError, match="hi"):
        K.check_window_ops("model", ek, g2, gd)


def _model_rebuild_output(c):
    """What a correct device returns for ring c, from the model."""
    R, e = K.rebuild_cases(), K.rebuild_expectations()[c]
    h, n = R["hists"][c], e["n"]
    keys = np.full((4, 64), M.KEY_NONE, dtype=np.uint32)
    oi, od = np.zeros(16, dtype=np.int64), np.zeros(12)
    for j, nm in enumerate(("q1", "q3", "bu", "bl")):
        a, b = e[nm]
        w = h[a:b + 1]
        if nm == "bl":
            w, a = (~w)[::-1], n - (b + 1)
        keys[j, :len(w)] = w
        oi[RP.RB_I[nm]], oi[RP.RB_I[nm] + 1] = a, len(w)
    oi[RP.RB_I["qc"]], oi[RP.RB_I["qc"] + 1] = e["qc"]
    oi[RP.RB_I["klb"]], oi[RP.RB_I["kub"]], oi[RP.RB_I["ok"]] = e["klb"], e["kub"], 1
    for nm in ("A1", "A2", "lb", "ub", "ctr"):
        od[RP.RB_D[nm]] = e[nm]
    for j in range(2):
        od[RP.RB_D["qs1"] + j], od[RP.RB_D["qs2"] + j] = e["qs1"][j], e["qs2"][j]
    return keys, oi, od


def test_the_ring_checkers_bite():
    X = K.rebuild_expectations()
    c = next(i for i, e in enumerate(X) if e["n"] == 1500 and e["qc"][0] > 0)
    keys, oi, od = _model_rebuild_output(c)
    assert K.check_rebuild(c, keys, oi, od)[0] is None
    o2 = oi.copy()
    o2[RP.RB_I["qc"]] += 1                                              # one tail count off by one
    assert "tail counts" in K.check_rebuild(c, keys, o2, od)[0]
    k2 = keys.copy()
    k2[3, 0], k2[3, 1] = keys[3, 1], keys[3, 0] ^ 1
    assert "bl" in K.check_rebuild(c, k2, oi, od)[0]
    d2 = od.copy()
    d2[RP.RB_D["A1"]] += 1e-6 * max(1.0, abs(d2[RP.RB_D["A1"]]))
    assert "A1" in K.check_rebuild(c, keys, oi, d2)[0]
    # refill: the model's own answer passes, r0 off by one and a swapped pair do not
    R = K.refill_cases()
    c = next(i for i, nt in enumerate(R["notes"]) if nt["feature"] == "plain" and int(R["meta"][i][2]) == K.UP)
    r0_in, hi_in, _, k, n, ps, px, side = (int(v) for v in R["meta"][c])
    h = K.ring_hist_space(R["ring"][c], ps, px, side)
    s = min(max(k - 32 - r0_in, 0), hi_in - 1)
    r0, hi = r0_in + s, min(64, n - (r0_in + s))
    keys = np.full(64, M.KEY_NONE, dtype=np.uint32)
    keys[:hi] = h[r0:r0 + hi]
    assert K.check_refill(c, keys, r0, hi) is None
    assert K.check_refill(c, keys, r0 + 1, hi) is not None
    assert K.check_refill(c, keys, r0, hi_in - s + 3) is not None      # too short an extension (and keys beyond hi)
    assert K.check_refill(c, keys, r0, 0) is not None                  # a wrongly dropped window
    c = next(i for i, nt in enumerate(R["notes"]) if not nt["consistent"])
    assert K.check_refill(c, keys, 5, 20) is not None and K.check_refill(c, keys, 0, 0) is None


def test_moment_bounds_are_met_by_the_algorithm_alone():
    """clipped_moments restated in NumPy meets, on the very inputs and against the very exact reference the device is held to, the very
    bounds: mean within 4 eps (|A1| + |T1|) / n, sd within 8 eps m2 / var + 1e-15 relative (eps = 2^-53).  The rational reference
    agrees with mpmath at 400 bits."""
    C = K.moments_cases()
    ref = M.moments_reference(C)
    w = K.check_moments(*K.np_clipped_moments(C), C, ref)
    print("NumPy clipped_moments, worst ratio to the bound:", w)
    assert w["n_pos"] > 50_000 and w["n_zero"] > 1000
    assert {int(x) for x in np.unique(C["n"] % 4)} == {0, 1, 2, 3}
    assert (C["n"] == C["n_full"]).sum() > 10_000 and (C["n"] != C["n_full"]).sum() > 10_000
    for i in range(0, len(C["n"]), 97):
        a = M.clipped_moments_exact(*(C[k][i] for k in ("n", "lb", "ub", "A1", "A2", "T1", "T2")))
        b = M.clipped_moments_mpmath(*(C[k][i] for k in ("n", "lb", "ub", "A1", "A2", "T1", "T2")))
        assert a == b, (i, a, b)


def test_bound_keys_by_definition_on_the_cases():
    """The by-definition search (the smallest key whose value is >= lb / > ub) against the key and its predecessor, on every case."""
    B = K.bounds_cases()
    assert B.shape[1] > 150_000 and {int(x) for x in np.unique(B[0] % 4)} == {0, 1, 2, 3}
    _, _, lb, ub, _ = M.bounds_from_keys(B[0].astype(np.int64), B[1], B[2], B[3], B[4])
    assert np.isfinite(lb).all() and np.isfinite(ub).all() and (ub >= lb).all()
    klb, kub = K.bound_keys_by_definition(lb, ub)
    assert (M.key_f64(klb) >= lb).all() and (M.key_f64(klb - np.uint32(1)) < lb).all()
    free = kub > klb                                                     # (kub is clamped to klb where ub == lb leaves it below)
    assert (M.key_f64(kub) > ub).all() and (M.key_f64(kub[free] - np.uint32(1)) <= ub[free]).all()
    zero = (lb == 0.0) | (ub == 0.0)
    print("bounds cases:", B.shape[1], "; with a bound at zero:", int(zero.sum()))
    assert zero.sum() >= 100
