"""The step's shared arithmetic (dc_rl_amd/csrc/sdc_physics.hpp, the two division shortcuts of sdc_device.hpp), function by function
on the device, through tests/aux/physics_probe.hip -- a test-only translation unit over the real header, built with the library's flags.

Every test runs both constant sources (literals / the LDS table), asserts them bit-equal on every output, then holds one of them to a
high-precision reference: mpmath at 200 bits for the short transcendentals, the IEEE quotient for the divisions, the C oracle
(oracle/sdc_oracle.c, pinned to the reference's captures by tests/test_oracle_golden.py) for the chiller, rack, HVAC and battery.  The
inputs, references and bounds live in tests/physics_cases.py; tests/test_physics_probe.py proves them sound on the CPU.

Measured on MI355X (each test prints its figures; DESIGN.md section 2 carries the list):
  log2_pos_normal  max |err| 8.8e-16 on [2^-30, 2^30] (header: 3e-15 there), 9.1e-16 over [2^-1000, 2^1000]; 5.1e-16 beyond the final rounding
  exp2_plain 3.4e-16, exp_plain 3.5e-16 (both ranges; bound 8.9e-16); exp2_short 2.72e-10, the rise 2.71e-10 (bound 2.91e-10)
  sdc_div_const 0 mismatches in 3 025 917 cases; sdc_div_fast <= 1 ulp from the quotient in 400 000
  chiller 7.1e-16; rack power 0 (the oracle's bits), fan power 1.1e-15, outlet 2.71e-10 of the rise; hvac comp 6.6e-16, ct 1.7e-15,
  total_kw 1.5e-15, water equal at all 44 064 points; battery: 0.213 % excluded, bat_load / soc_after equal everywhere (the excluded
  included), energy / co2 4.3e-16 of e_nobat (6.1e-13 of the energy itself where the discharge nearly cancels it)
"""
import numpy as np
import pytest

from tests import physics_cases as K
from tests import physics_probe as PP

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _by_set(name, inputs):
    return {k: PP.run_both(name, v)[0] for k, v in inputs.items()}


# ---- the short transcendentals vs mpmath ---------------------------------------------------------------------------------------------------
def test_log2_pos_normal_vs_mpmath():
    """|err| <= 0.5 ulp(result) + 1e-15 on every set (the final rounding no fp64 routine avoids + the roundings of the fractional part,
    <= 0.5 in magnitude); the header's 3e-15 is a bound on the rack model's range [2^-30, 2^30]."""
    got = _by_set("log2_pos_normal", K.log2_inputs())
    worst = K.check_log2(got, "device")
    print("log2_pos_normal max |err| by set:", {k: f"{v:.3g}" for k, v in worst.items()},
          "; on the rack range %.3g against the header's %.1g" % (worst["rack"], K.HEADER_LOG2_RACK_BOUND))
    assert worst["rack"] <= K.HEADER_LOG2_RACK_BOUND
    # the excess over the final rounding alone, everywhere
    for name, refs in K.log2_refs().items():
        err = K.abs_errors(got[name], refs)
        print(f"  set {name}: max (|err| - 0.5 ulp) = {(err - 0.5 * np.spacing(np.abs(K.refs_as_float(refs)))).max():.3g}")
    assert got["one"][50] == 0.0 and (got["binade"][81:162] == np.arange(-40.0, 41.0)).all()      # log2 of 2^k is exactly k


def test_exp2_plain_vs_mpmath():
    got = _by_set("exp2_plain", K.exp2_inputs())
    worst = K.check_rel(got, K.exp2_inputs(), K.exp2_refs(), K.EXP_PLAIN_REL, "device exp2_plain")
    print("exp2_plain max rel err by set:", {k: f"{v:.3g}" for k, v in worst.items()}, "bound %.3g" % K.EXP_PLAIN_REL)
    ints = K.exp2_inputs()["integers"]
    assert np.array_equal(got["integers"], np.exp2(ints))


def test_exp_plain_vs_mpmath():
    got = _by_set("exp_plain", K.exp_inputs())
    worst = K.check_rel(got, K.exp_inputs(), K.exp_refs(), K.EXP_PLAIN_REL, "device exp_plain")
    print("exp_plain max rel err by set:", {k: f"{v:.3g}" for k, v in worst.items()}, "bound %.3g" % K.EXP_PLAIN_REL)
    assert got["sigmoid"][-1] == 1.0


def test_exp2_short_and_rise_vs_mpmath():
    """The degree-8 Taylor remainder at |f| = ln2 / 2 relative to e^f bounds exp2_short; the rise P^1.096 / V^0.824 as the header's own
    rack_outlet forms it (inlet 0, k_outlet 1: the probe returns rise + (-14.01), the comparison adds the 14.01 back in 200 bits)
    stays under the same bound against mpmath.power."""
    bound = K.exp2_short_bound()
    got = _by_set("exp2_short", K.exp2_inputs())
    worst = K.check_rel(got, K.exp2_inputs(), K.exp2_refs(), bound, "device exp2_short")
    p, v = K.rise_inputs()
    out = PP.run_both("rise", p, v)[0]
    err = K.rel_errors(out, K.rise_refs(), offset=14.01)
    print("exp2_short max rel err by set:", {k: f"{v:.3g}" for k, v in worst.items()}, "rise %.4g, bound %.4g" % (err.max(), bound))
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), float(err.max()), p[np.argmax(err)], v[np.argmax(err)])


# ---- the two division shortcuts ------------------------------------------------------------------------------------------------------------
def test_div_const_is_the_ieee_quotient_on_its_run_time_divisors():
    total = 0
    for name, (x, c) in K.div_const_cases().items():
        got = PP.run_both("div_const", x, c, 1.0 / c)[0]
        ref = x / c
        bad = _bits(got) != _bits(ref)
        total += len(x)
        print(f"sdc_div_const, {name}: {len(x)} cases, {int(bad.sum())} mismatches")
        assert not bad.any(), (name, int(bad.sum()), x[bad][:5], c[bad][:5], got[bad][:5], ref[bad][:5])
    print("sdc_div_const:", total, "cases, 0 mismatches")


def test_div_fast_is_within_two_ulp_of_the_quotient():
    a, b = K.div_fast_cases()
    got = PP.run_both("div_fast", a, b)[0]
    ref = a / b
    ulps = np.abs(got - ref) / np.spacing(np.abs(ref))
    print(f"sdc_div_fast: {len(a)} cases, max {ulps.max():.2f} ulp from the float64 quotient, {(ulps > 0).mean():.3%} not equal to it")
    assert np.isfinite(got).all() and ulps.max() <= 2.0, (float(ulps.max()), a[np.argmax(ulps)], b[np.argmax(ulps)])


# ---- chiller, rack, HVAC, battery vs the oracle -----------------------------------------------------------------------------------------
def _rel(got, ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref != 0, np.abs(got - ref) / np.abs(ref), np.where(got == 0, 0.0, np.inf))


def test_chiller_power_vs_oracle():
    cap, load, amb, ref = K.chiller_cases()
    got = PP.run_both("chiller_power", cap, load, amb)[0]
    assert np.array_equal(got == 0, ref == 0), "zero / non-zero differs from the oracle"
    err = _rel(got, ref)
    ratio = load / (cap * K.chiller_cap_rat(amb))
    print(f"chiller_power: {len(ref)} points, max rel err {err.max():.3g}; zero at {int((ref == 0).sum())}; load / avail < 0.05 at "
          f"{int(((ratio > 0) & (ratio < 0.05)).sum())}, saturated at {int((ratio >= 1).sum())}")
    assert err.max() <= 1e-13, (float(err.max()), cap[np.argmax(err)], load[np.argmax(err)], amb[np.argmax(err)])


def test_rack_point_and_the_lane_per_env_composition_vs_oracle():
    d = K.rack_cases()
    a = PP.run_both("rack_point", *d["rows"])
    b = PP.run_both("rack_wide", *d["rows"])
    assert np.array_equal(_bits(a), _bits(b)), "rack_point and the lane-per-env kernel's composition differ"
    pc, pf, out, plain, inlet = a
    err_p = _rel(pc + pf, d["p_it"])
    s = d["second"]
    err_c = _rel(pc[s], d["pcpu"][s])
    err_f = _rel(pf[s], d["p_it"][s] - d["pcpu"][s])      # (a difference of the oracle's two runs: its own rounding is ~1e-16 of P_it)
    rise = d["outlet"] - inlet + 14.01                     # k_outlet * P^1.096 / V^0.824, kelvin
    err_o = np.abs(out - d["outlet"])
    bound = K.exp2_short_bound()
    print(f"rack: {len(pc)} points, power max rel err {err_p.max():.3g} (cpu {err_c.max():.3g}, fan {err_f.max():.3g}); outlet max abs err "
          f"{err_o.max():.3g} K, max err / rise {np.max(err_o / rise):.3g} (bound {bound:.3g}); outlet-delta flag set at "
          f"{int((d['fault'] & 1 != 0).sum())}")
    assert err_p.max() <= 1e-13 and err_c.max() <= 1e-13 and err_f.max() <= 1e-13
    # the CPU power is the oracle's very sequence of IEEE operations (the load's shift through the exact division by 100): the same bits,
    # as long as no multiply-add of it is contracted
    assert np.array_equal(_bits(pc[s]), _bits(d["pcpu"][s])), "rack CPU power: not the oracle's bits"
    assert (err_o <= bound * rise).all(), float(np.max(err_o / rise))
    # a valid config's powers and air flows are plain numbers: the oracle's are finite and positive on the whole grid
    assert np.isfinite(d["outlet"]).all() and (d["p_it"] > 0).all()
    assert (plain == 1.0).all()
    flag = (out - inlet < 2) | (plain != 1.0)              # as both callers raise SDC_FAULT_OUTLET_DELTA
    assert np.array_equal(flag, d["fault"] & 1 != 0)
    assert 0 < flag.sum() < len(flag)
    sa = np.clip(d["supply"], 3.8, 5.3)
    assert np.array_equal(inlet, sa + d["stpt"])


def test_hvac_water_vs_oracle():
    d = K.hvac_cases()
    o = d["out"]                   # {P_it, CT, compressor, avg_return, mean_outlet, water, Q_cooling, sum_outlet}
    got = PP.run_both("hvac_water", d["c_air"], d["rho_air"], d["ct_fan_ref_p"], d["crac_supply_pu"], 1.0 / d["rho_air"], 1.0 / d["ctafr"],
                      o[:, 0], o[:, 3], d["stpt"], d["amb"], d["wb"])
    comp, ct, water, total_kw = got
    assert np.array_equal(ct == 0, o[:, 1] == 0), "ct == 0 differs from the oracle"
    assert np.array_equal(comp == 0, o[:, 2] == 0)
    ref_total = (o[:, 0] + o[:, 1] + o[:, 2]) / 1e3
    e_comp, e_ct, e_tot = _rel(comp, o[:, 2]), _rel(ct, o[:, 1]), _rel(total_kw, ref_total)
    # the oracle's own w * 250 * 1e4 before np.round(., 4), from its CRAC return temperature
    w = 0.044 * d["wb"] + (0.3528 * (o[:, 3] - d["stpt"]) + 0.101)
    clamped = w < 0
    w = np.where(clamped, 0.0, w)
    w = w + w * 0.01
    pre = ((w * 1000) / 4) * 1e4
    safe = np.abs((pre - np.floor(pre)) - 0.5) >= 1e-3
    x = (o[:, 6] / (d["c_air"] * np.maximum(50 - (d["amb"] - d["stpt"]), 1)) / d["rho_air"]) / d["ctafr"]
    print(f"hvac_water: {len(comp)} points; max rel err comp {e_comp.max():.3g}, ct {e_ct.max():.3g}, total_kw {e_tot.max():.3g}; water "
          f"compared at {int(safe.sum())} ({int((~safe).sum())} within 1e-3 of a tie), w < 0 at {int(clamped.sum())}, ct == 0 at "
          f"{int((ct == 0).sum())}, fan saturated at {int((x >= 1).sum())} / below at {int((x < 1).sum())}, dlt clamped at "
          f"{int((50 - (d['amb'] - d['stpt']) <= 1).sum())}")
    assert e_comp.max() <= 1e-13 and e_ct.max() <= 1e-13 and e_tot.max() <= 1e-13
    assert np.array_equal(_bits(water[safe]), _bits(o[safe, 5]))
    assert clamped.sum() > 100 and (~clamped).sum() > 100 and safe.mean() > 0.99


def test_battery_step_vs_oracle():
    """bat_load and soc_after bit-equal, the flag mask equal on every point, energy and co2 to 1e-13.  Excluded from the bit comparisons:
    points whose own pre-rounding rate * 1e4 or load * 1e8 (the oracle's) lies within 1e-3 of a half-integer -- at most 0.5 % of the grid.
    energy = e_nobat -/+ the battery's share: 1e-13 is taken against the larger operand, e_nobat (and e_nobat * ci for co2) -- where the
    discharge is limited by dcload / 4 and the SoC nears 1, energy is e_nobat (1 - tu) with 1 / (1 - tu) up to 1809, and the one ulp by
    which two correct exps may differ in the sigmoid is 2e-13 of that difference.  The plain relative figure is printed."""
    b = K.battery_cases()
    ref = b["ref"]
    got = PP.run_both("battery_step", b["a"], b["load"], b["cap"], 1.0 / b["cap"], b["total_kw"], b["ci"])
    e_nobat, energy, co2, soc_after, load_after, flag = got
    ex = K.battery_excluded(ref)
    share = float(ex.mean())
    assert share <= K.BATTERY_MAX_EXCLUDED, share
    assert np.array_equal(flag.astype(np.uint32), b["fault"]), "fault mask differs from the oracle"
    keep = ~ex
    bad_load = _bits(load_after[keep]) != _bits(ref[keep, 0])
    bad_soc = _bits(soc_after[keep]) != _bits(ref[keep, 4])
    assert np.array_equal(_bits(e_nobat), _bits(ref[:, 1]))
    scale_e = np.maximum(np.abs(ref[:, 2]), np.abs(ref[:, 1]))
    err_e = np.abs(energy - ref[:, 2]) / scale_e
    err_c = np.abs(co2 - ref[:, 3]) / (scale_e * b["ci"])
    with np.errstate(divide="ignore", invalid="ignore"):
        plain_e = np.where(ref[:, 2] != 0, np.abs(energy - ref[:, 2]) / np.abs(ref[:, 2]), 0.0)
    print(f"battery_step: {len(ex)} points, {int(ex.sum())} excluded ({100 * share:.3f} %); bat_load mismatches {int(bad_load.sum())}, "
          f"soc_after {int(bad_soc.sum())}; among the excluded {int((_bits(load_after[ex]) != _bits(ref[ex, 0])).sum())} differ; energy "
          f"max err {err_e.max():.3g}, co2 {err_c.max():.3g} (of e_nobat); energy relative to itself {plain_e.max():.3g}")
    assert not bad_load.any(), (b["a"][keep][bad_load][:5], b["load"][keep][bad_load][:5], b["cap"][keep][bad_load][:5])
    assert not bad_soc.any()
    assert err_e[keep].max() <= 1e-13 and err_c[keep].max() <= 1e-13
