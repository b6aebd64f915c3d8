"""What the host derives before anything is uploaded (csrc/sdc_setup.hpp), without a GPU: the header compiled by g++ alone into a
program that reads requests and prints what the header answers, held to
  * a restatement in Python that shares no text with the header (dict-ordered distinct tuples, sorts, names instead of offsets), over
    the shipped configs, the rack cases of tests/step_paths.py and seeded random rack tables,
  * the figures written out by hand in DESIGN.md section 4.21 (geometry, thresholds, refusal texts),
  * and the same program built with -fsanitize=address,undefined, run over the same input.

A request line and what it calls (doubles travel as C99 hex floats, so every bit arrives and returns):
  K n_envs episode_steps hist_cap queue_max_len n_locations n_dc_configs env_index_base reward_method[3] policy[3]
                        sdc_check_config -> after_device | message (- : taken)
  G n_envs episode_steps debug_flags
                        sdc_geometry -> lw qstride rq_max sweep_blocks qcum_t hist_t has_feat feat_waves feat_use_sma feat_lds_bytes
  Z n                   n configs, none set
  D slot n_racks listed (cpus full idle supply return)[listed] scalars[18]
                        sdc_derive_dc -> ! message, or the derived fields | the rack classes; the config is stored in `slot`
  B n_envs assigned ids[n_envs if assigned]
                        sdc_config_tables over the stored configs -> facts | per config's SdcWideCfg | prm_env | prm_cfg
  M n_envs ids[n_envs]  sdc_racks_max"""
import random
import struct
import subprocess

import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import dc_config
from tests import step_paths

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "sdc_setup.hpp"
static double sdc_dc_params::*const SCAL[18] = {
    &sdc_dc_params::m_cpu, &sdc_dc_params::c_cpu, &sdc_dc_params::rs_cpu, &sdc_dc_params::m_fan, &sdc_dc_params::c_fan,
    &sdc_dc_params::rs_fan, &sdc_dc_params::itfan_ref_p, &sdc_dc_params::itfan_ref_v_ratio, &sdc_dc_params::it_fan_full_load_v,
    &sdc_dc_params::c_air, &sdc_dc_params::rho_air, &sdc_dc_params::crac_supply_pu, &sdc_dc_params::ct_fan_ref_p, &sdc_dc_params::ctafr,
    &sdc_dc_params::min_temp, &sdc_dc_params::max_temp, &sdc_dc_params::init_setpoint, &sdc_dc_params::bat_capacity_mwh};
static bool ints(std::vector<int>& v, const size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; i++)
    if (std::scanf("%d", &v[i]) != 1) return false;
  return true;
}
static void put(const double* x, const size_t n) {
  for (size_t i = 0; i < n; i++) std::printf(" %a", x[i]);
}
static void put(const int* x, const size_t n) {
  for (size_t i = 0; i < n; i++) std::printf(" %d", x[i]);
}
int main() {
  std::vector<SdcDcDev> dc;
  std::vector<unsigned char> set;
  std::vector<int> v;
  char tag;
  while (std::scanf(" %c", &tag) == 1) {
    if (tag == 'K') {
      if (!ints(v, 13)) return 2;
      sdc_config c{};
      c.n_envs = v[0], c.episode_steps = v[1], c.hist_cap = v[2], c.queue_max_len = v[3], c.n_locations = v[4], c.n_dc_configs = v[5];
      c.env_index_base = v[6];
      for (int a = 0; a < 3; a++) c.reward_method[a] = v[7 + a], c.policy[a] = v[10 + a];
      const SdcRefusal r = sdc_check_config(c);
      std::printf("%d | %s\n", (int)r.after_device, r.msg ? r.msg : "-");
    } else if (tag == 'G') {
      if (!ints(v, 3)) return 2;
      sdc_config c{};
      c.n_envs = v[0], c.episode_steps = v[1], c.debug_flags = v[2];
      const SdcGeometry g = sdc_geometry(c);
      std::printf("%d %d %d %d %d %d %d %d %d %zu\n", g.lw, g.qstride, g.rq_max, g.sweep_blocks, (int)g.mirrors.qcum_t, (int)g.mirrors.hist_t,
                  (int)g.has_feat, g.feat_waves, g.feat_use_sma, g.feat_lds_bytes);
    } else if (tag == 'Z') {
      if (!ints(v, 1)) return 2;
      dc.assign((size_t)v[0], SdcDcDev{});
      set.assign((size_t)v[0], 0);
      std::printf("-\n");
    } else if (tag == 'D') {
      if (!ints(v, 3) || v[2] < 0 || v[2] > SDC_MAX_RACKS || v[0] < 0 || (size_t)v[0] >= dc.size()) return 2;
      const int slot = v[0];
      sdc_dc_params p{};
      p.n_racks = v[1];
      for (int r = 0; r < v[2]; r++)
        if (std::scanf("%la %la %la %la %la", &p.rack_n[r], &p.rack_full[r], &p.rack_idle[r], &p.rack_supply[r], &p.rack_return[r]) != 5) return 2;
      for (int i = 0; i < 18; i++)
        if (std::scanf("%la", &(p.*SCAL[i])) != 1) return 2;
      SdcDcDev e;
      if (const char* why = sdc_derive_dc(p, e)) {
        std::printf("! %s\n", why);
        continue;
      }
      dc[(size_t)slot] = e;
      set[(size_t)slot] = 1;
      std::printf("%d", (int)(std::memcmp(&e.p, &p, sizeof(p)) == 0));
      put(&e.rc_n_racks, 5);
      put(&e.k_outlet, 1), put(&e.n_racks_f, 1), put(&e.ret_sum, 1);
      std::printf(" |");
      const SdcRackClasses& rc = e.rc;
      put(&rc.n_grp, 1), put(&rc.n_cls, 1), put(rc.grp_begin, SDC_MAX_RACK_CLS + 1), put(rc.cls_of_rack, 32), put(rc.pad, 21);
      put(rc.grp_n, SDC_MAX_RACK_CLS), put(rc.grp_supply, SDC_MAX_RACK_CLS), put(rc.cls_full, SDC_MAX_RACK_CLS), put(rc.cls_idle, SDC_MAX_RACK_CLS);
      std::printf("\n");
    } else if (tag == 'B') {
      if (!ints(v, 2)) return 2;
      const int n_envs = v[0], assigned = v[1];
      if (assigned && !ints(v, (size_t)n_envs)) return 2;
      const SdcConfigTables t = sdc_config_tables(dc.data(), set.data(), (int)dc.size(), assigned ? v.data() : nullptr, n_envs);
      const SdcConfigFacts& f = t.facts;
      std::printf("%d %d %d %d %d %d %d |", f.racks_cfg0, f.rack_cls_cfg0, (int)f.prm_env_ok, f.racks_max, (int)f.wide_gen_ok, t.wide_max_cls,
                  t.wide_max_racks4);
      for (const SdcWideCfg& w : t.wide) {
        const int m[6] = {w.n_cls, w.n_racks, (int)w.map[0], (int)w.map[1], (int)w.map[2], (int)w.map[3]};
        put(m, 6), put(w.scal, WC_SCAL_COUNT), put(&w.cls[0][0], 4 * SDC_WIDE_MAX_CLS), put(w.pad, 2);
      }
      std::printf(" |");
      put(t.prm_env.data(), t.prm_env.size());
      std::printf(" |");
      put(t.prm_cfg.data(), t.prm_cfg.size());
      std::printf("\n");
    } else if (tag == 'M') {
      if (!ints(v, 1) || !ints(v, (size_t)v[0])) return 2;
      std::printf("%d\n", sdc_racks_max(dc.data(), v.data(), (int)v.size()));
    } else {
      return 3;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """the driver built by g++ alone (no HIP on the include path): plain, and with the address and undefined-behaviour sanitizers"""
    d = tmp_path_factory.mktemp("setup")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + L.CSRC, str(src)]
    plain, san = str(d / "driver"), str(d / "driver_san")
    subprocess.run(base + ["-O1", "-o", plain], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san], check=True)
    return plain, san


@pytest.fixture(scope="module")
def ask(drivers):
    """request lines -> answer lines; every request runs on both builds of the driver, which must agree"""
    def run(lines):
        outs = []
        for exe in drivers:
            out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
            assert out.returncode == 0, (exe, out.returncode, out.stderr[-2000:])
            outs.append(out.stdout.splitlines())
        assert outs[0] == outs[1] and len(outs[0]) == len(lines)
        return outs[0]
    return run


# ---- requests ----------------------------------------------------------------------------------------------------------------------------
SCALARS = ("m_cpu", "c_cpu", "rs_cpu", "m_fan", "c_fan", "rs_fan", "itfan_ref_p", "itfan_ref_v_ratio", "it_fan_full_load_v", "c_air", "rho_air",
           "crac_supply_pu", "ct_fan_ref_p", "ctafr", "min_temp", "max_temp", "init_setpoint", "bat_capacity")
RACK_COLS = ("rack_n", "rack_full", "rack_idle", "rack_supply", "rack_return")


def hx(x):
    return float(x).hex()


def bits(x):
    return struct.pack("<d", float(x))


def derive_line(slot, p, n_racks=None):
    listed = len(p["rack_n"])
    racks = [hx(p[c][r]) for r in range(listed) for c in RACK_COLS]
    return " ".join(["D", str(slot), str(listed if n_racks is None else n_racks), str(listed)] + racks + [hx(p[s]) for s in SCALARS])


def parse_derived(ln):
    head, rc = ln.split("|")
    head, rc = head.split(), rc.split()
    ints, dbl = [int(x) for x in rc[:64]], [float.fromhex(x) for x in rc[64:]]
    return dict(p_kept=int(head[0]), rc=[float.fromhex(x) for x in head[1:6]], k_outlet=float.fromhex(head[6]), n_racks_f=float.fromhex(head[7]),
                ret_sum=float.fromhex(head[8]), n_grp=ints[0], n_cls=ints[1], grp_begin=ints[2:11], cls_of_rack=ints[11:43], pad=ints[43:64],
                grp_n=dbl[0:8], grp_supply=dbl[8:16], cls_full=dbl[16:24], cls_idle=dbl[24:32])


def parse_tables(ln):
    f, w, e, c = ln.split("|")
    f, w = [int(x) for x in f.split()], w.split()
    wide = []
    for k in range(0, len(w), 62):
        m, d = [int(x) for x in w[k:k + 6]], [float.fromhex(x) for x in w[k + 6:k + 62]]
        wide.append(dict(n_cls=m[0], n_racks=m[1], map=[x & 0xFFFFFFFF for x in m[2:6]], scal=d[0:6], cls=[d[6 + 4 * j:10 + 4 * j] for j in range(12)],
                         pad=d[54:56]))
    rows = lambda part: [[float.fromhex(x) for x in part.split()[k:k + 32]] for k in range(0, len(part.split()), 32)]
    return dict(racks_cfg0=f[0], rack_cls_cfg0=f[1], prm_env_ok=f[2], racks_max=f[3], wide_gen_ok=f[4], wide_max_cls=f[5], wide_max_racks4=f[6],
                wide=wide, prm_env=rows(e), prm_cfg=rows(c))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def kinds(p):
    """the racks' (cpus, supply approach, full load, idle) kinds, each once, as first met; and every rack's kind"""
    per_rack = list(zip(p["rack_n"], p["rack_supply"], p["rack_full"], p["rack_idle"]))
    return list(dict.fromkeys(per_rack)), per_rack


def want_rack_classes(p):
    """SdcRackClasses: kinds sorted (stably) by the first appearance of their (cpus, supply approach) pair; nothing beyond 32 racks / 8 kinds"""
    met, per_rack = kinds(p)
    if len(per_rack) > 32 or len(met) > 8:
        return dict(n_grp=0, n_cls=0, grp_begin=[0] * 9, cls_of_rack=[0] * 32, grp_n=[0.0] * 8, grp_supply=[0.0] * 8, cls_full=[0.0] * 8,
                    cls_idle=[0.0] * 8)
    pairs = list(dict.fromkeys((k[0], k[1]) for k in met))
    ordered = sorted(met, key=lambda k: pairs.index((k[0], k[1])))
    fill = lambda xs, n, zero: list(xs) + [zero] * (n - len(xs))
    begins = [sum(1 for k in ordered if pairs.index((k[0], k[1])) < g) for g in range(len(pairs) + 1)]
    return dict(n_grp=len(pairs), n_cls=len(ordered), grp_begin=fill(begins, 9, 0), cls_of_rack=fill([ordered.index(k) for k in per_rack], 32, 0),
                grp_n=fill([a for a, _ in pairs], 8, 0.0), grp_supply=fill([b for _, b in pairs], 8, 0.0),
                cls_full=fill([k[2] for k in ordered], 8, 0.0), cls_idle=fill([k[3] for k in ordered], 8, 0.0))


def want_wide(p, derived):
    """SdcWideCfg: the kinds as first met, a nibble per rack; None beyond 32 racks / 12 kinds"""
    met, per_rack = kinds(p)
    if len(per_rack) > 32 or len(met) > 12:
        return None
    word = lambda k: sum(met.index(per_rack[r]) << (4 * (r - 8 * k)) for r in range(8 * k, min(8 * k + 8, len(per_rack))))
    scal = [derived["ret_sum"], derived["rc"][0], p["ct_fan_ref_p"], derived["rc"][3], p["bat_capacity"], derived["rc"][4]]
    return dict(n_cls=len(met), n_racks=len(per_rack), map=[word(k) for k in range(4)], scal=scal,
                cls=[list(k) for k in met] + [[0.0] * 4] * (12 - len(met)), pad=[0.0, 0.0])


UNIFORM = ("m_cpu", "c_cpu", "rs_cpu", "m_fan", "c_fan", "rs_fan", "itfan_ref_p", "itfan_ref_v_ratio", "it_fan_full_load_v", "c_air", "rho_air",
           "crac_supply_pu", "min_temp", "max_temp")      # (and what is computed from them: two reciprocals, k_outlet)


def want_row(p, d):
    """a config's 32-double row: the 18 scalars, the five reciprocals, k_outlet, the rack count, the return sum, zeros"""
    return [p[s] for s in SCALARS] + d["rc"] + [d["k_outlet"], d["n_racks_f"], d["ret_sum"]] + [0.0] * 6


def same_bits(a, b):
    flat = lambda x: [flat(y) for y in x] if isinstance(x, (list, tuple)) else (bits(x) if isinstance(x, float) else x)
    return flat(a) == flat(b)


def check_config(ask_derived, p):
    """one config through sdc_derive_dc against the restatement -> the parsed answer"""
    d = ask_derived
    assert d["p_kept"] == 1 and d["pad"] == [0] * 21
    divisors = [float(len(p["rack_n"])), p["itfan_ref_v_ratio"], p["rho_air"], p["ctafr"], p["bat_capacity"]]
    assert same_bits(d["rc"], [1.0 / x for x in divisors])
    assert same_bits(d["k_outlet"], 1.918 / (p["c_air"] * p["rho_air"] * 0.526)) and d["n_racks_f"] == len(p["rack_n"])
    total = 0.0
    for x in p["rack_return"]:
        total += x
    assert same_bits(d["ret_sum"], total)
    want = want_rack_classes(p)
    for key, val in want.items():
        assert same_bits(d[key], val), (key, d[key], val)
    return d


def shipped(name):
    p = dc_config.size_datacenter(name, 1)
    return {k: ([float(x) for x in p[k]] if k in RACK_COLS else float(p[k])) for k in RACK_COLS + SCALARS}


def with_racks(p, n_racks, n_classes):
    """tests/test_gpu_kernel_reach.py rack_config's rack tables: the shipped lists repeated, or one server type with exactly n_classes
    distinct supply approach temperatures"""
    q = dict(p)
    for c in RACK_COLS:
        q[c] = (p[c] * (n_racks // len(p[c]) + 1))[:n_racks]
    if n_classes is not None:
        q["rack_supply"] = [5.0 + 0.1 * (r % n_classes) for r in range(n_racks)]
        q["rack_return"] = [-2.5] * n_racks
        q["rack_n"], q["rack_full"], q["rack_idle"] = [float(int(p["rack_n"][0]))] * n_racks, [130.0] * n_racks, [10.0] * n_racks
    return q


def one_bit_up(x):
    return struct.unpack("<d", struct.pack("<q", struct.unpack("<q", struct.pack("<d", x))[0] + 1))[0]


# ---- configs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,racks,classes,groups", [("dc_config.json", 20, 7, 2), ("dc_config_r16.json", 16, 8, 4),
                                                        ("dc_config_r25.json", 25, 11, 6)])
def test_shipped_configs(ask, name, racks, classes, groups):
    p = shipped(name)
    out = ask(["Z 1", derive_line(0, p), "B 4 0"])
    d = check_config(parse_derived(out[1]), p)
    met, per_rack = kinds(p)
    assert len(per_rack) == racks and len(met) == classes and len(dict.fromkeys((k[0], k[1]) for k in met)) == groups
    fits = classes <= 8
    assert (d["n_cls"], d["n_grp"]) == ((classes, groups) if fits else (0, 0))
    t = parse_tables(out[2])
    assert t["racks_cfg0"] == racks and t["rack_cls_cfg0"] == d["n_cls"] and t["wide_gen_ok"] == 1 and t["prm_env_ok"] == 0
    assert t["wide_max_cls"] == classes and t["wide_max_racks4"] == (racks + 3) // 4 * 4 and t["prm_env"] == [] and t["prm_cfg"] == []
    assert same_bits(t["wide"], [want_wide(p, d)])


@pytest.mark.parametrize("racks,classes", step_paths.RACK_CASES)
def test_rack_cases_of_the_step_paths(ask, racks, classes):
    p = with_racks(shipped("dc_config.json"), racks, classes)
    out = ask(["Z 1", derive_line(0, p), "B 2 0"])
    d = check_config(parse_derived(out[1]), p)
    t = parse_tables(out[2])
    k = len(kinds(p)[0])
    assert classes is None or k == classes
    assert (d["n_cls"] > 0) == (racks <= 32 and k <= 8) and t["rack_cls_cfg0"] == d["n_cls"] and t["racks_cfg0"] == racks
    assert t["wide_gen_ok"] == int(racks <= 32 and k <= 12)
    # ... as tests/step_paths.py expects a batch to land: no class table -> never the common form; no wide form -> never the general one
    land = step_paths.expected_mapping(step_paths.WIDE, racks, k)
    assert land == ("general" if racks > 32 else "wide" if d["n_cls"] else "wide_gen" if t["wide_gen_ok"] else "pair")
    if t["wide_gen_ok"]:
        assert same_bits(t["wide"], [want_wide(p, d)])
    else:
        assert t["wide"] == [] and t["wide_max_cls"] == 0 and t["wide_max_racks4"] == 0


def test_random_rack_tables(ask):
    """few distinct values per column, so that kinds repeat, groups interleave and the capacities 8 / 12 are crossed"""
    rng = random.Random(20)
    base = shipped("dc_config.json")
    cases = []
    for _ in range(200):
        n = rng.choice([1, 2, 7, 8, 9, 12, 13, 20, 31, 32, 33, 64])
        pick = lambda vals: [rng.choice(vals[:rng.randint(1, len(vals))]) for _ in range(n)]
        p = dict(base)
        p["rack_n"], p["rack_supply"] = pick([18.0, 20.0, 22.0]), pick([5.0, 5.1, 5.3, -0.0, 0.0])
        p["rack_full"], p["rack_idle"] = pick([130.0, 170.0, 200.0]), pick([10.0, 60.0])
        p["rack_return"] = [rng.uniform(-4.0, 0.0) for _ in range(n)]
        cases.append(p)
    lines = ["Z 1"]
    for p in cases:
        lines += [derive_line(0, p), "B 1 0"]
    out = ask(lines)
    seen = set()
    for i, p in enumerate(cases):
        d = check_config(parse_derived(out[1 + 2 * i]), p)
        t = parse_tables(out[2 + 2 * i])
        w = want_wide(p, d)
        assert t["wide_gen_ok"] == int(w is not None) and same_bits(t["wide"], [w] if w else [])
        seen.add((d["n_cls"] > 0, w is not None, d["n_grp"] > 1))
    assert {(True, True, True), (True, True, False), (False, True, False), (False, False, False)} <= seen


def test_reciprocals_are_exact_or_refused(ask):
    p = shipped("dc_config.json")
    text = ("! sdc_set_dc_params: n_racks, itfan_ref_v_ratio, rho_air, ctafr and bat_capacity_mwh must be positive, finite, and not have "
            "an all-ones significand")
    all_ones = float.fromhex("0x1.fffffffffffffp+3")
    lines = ["Z 1"]
    for key in ("itfan_ref_v_ratio", "rho_air", "ctafr", "bat_capacity"):
        for bad in (0.0, -1.5, float("inf"), float("nan"), all_ones, -0.0):
            lines.append(derive_line(0, dict(p, **{key: bad})))
    assert ask(lines)[1:] == [text] * 24
    # the rack count is the fifth divisor: 0 and 65 are out of range before it is one, and no rack count in range has an all-ones
    # significand that 1 / n could miss (31 and 63 are exact in fp64: their significands are five and six ones, not 52)
    out = ask(["Z 1", derive_line(0, p, 0), derive_line(0, p, -3), derive_line(0, with_racks(p, 64, None), 65), "B 1 0"])
    assert out[1:4] == ["! sdc_set_dc_params: n_racks must be in [1, 64]"] * 3
    assert parse_tables(out[4])["racks_cfg0"] == 0      # (a refused config is not set)
    rng = random.Random(5)
    cases = [dict(with_racks(p, rng.randint(1, 64), None), itfan_ref_v_ratio=rng.uniform(0.1, 9.0), rho_air=rng.uniform(0.5, 2.0),
                  ctafr=rng.uniform(1.0, 1e4), bat_capacity=rng.choice([rng.uniform(0.01, 50.0), 5e-324, 1.7e308])) for _ in range(40)]
    for q, ln in zip(cases, ask(["Z 1"] + [derive_line(0, q) for q in cases])[1:]):
        check_config(parse_derived(ln), q)


# ---- batches of configs ------------------------------------------------------------------------------------------------------------------
def test_several_configs(ask):
    a, b, c = shipped("dc_config.json"), shipped("dc_config_r16.json"), shipped("dc_config_r25.json")
    ids = [1, 0, 1, 1, 0, 1]
    out = ask(["Z 3", "B 6 0", derive_line(1, b), "B 6 0", derive_line(0, a), "B 6 1 " + " ".join(map(str, ids)), derive_line(2, c), "B 6 0",
               "B 6 1 " + " ".join(map(str, ids)), "B 6 1 2 2 0 0 1 2", "M 6 1 1 1 1 1 1", "M 6 1 0 2 1 1 0"])
    da, db, dc = parse_derived(out[4]), parse_derived(out[2]), parse_derived(out[6])
    none, only_b, a_and_b, unassigned, full, other = (parse_tables(out[i]) for i in (1, 3, 5, 7, 8, 9))
    # nothing set; config 0 not set; one config missing: neither table, config 0's facts as soon as it is set
    assert (none["racks_cfg0"], only_b["racks_cfg0"], a_and_b["racks_cfg0"], a_and_b["rack_cls_cfg0"]) == (0, 0, 20, 7)
    for t in (none, only_b, a_and_b):
        assert t["prm_env_ok"] == 0 and t["wide_gen_ok"] == 0 and t["wide"] == [] and t["prm_env"] == [] and t["racks_max"] == 0
    # every config set: the wide form whatever the assignment, the envs' rows only once they are assigned
    assert unassigned["wide_gen_ok"] == 1 and unassigned["prm_env_ok"] == 0 and unassigned["prm_env"] == []
    wide = [want_wide(p, d) for p, d in ((a, da), (b, db), (c, dc))]
    rows = [want_row(p, d) for p, d in ((a, da), (b, db), (c, dc))]
    for t, assigned in ((full, ids), (other, [2, 2, 0, 0, 1, 2])):
        assert t["wide_gen_ok"] == 1 and t["prm_env_ok"] == 1 and (t["wide_max_cls"], t["wide_max_racks4"]) == (11, 28)
        assert same_bits(t["wide"], wide) and same_bits(t["prm_cfg"], rows) and same_bits(t["prm_env"], [rows[i] for i in assigned])
    # racks_max is over the configs IN USE: the assignment that leaves the 25-rack config out stays at 20
    assert full["racks_max"] == 20 and other["racks_max"] == 25 and out[10] == "16" and out[11] == "25"
    # one config: never the envs' rows (the kernels read the config itself)
    assert parse_tables(ask(["Z 1", derive_line(0, a), "B 3 1 0 0 0"])[2])["prm_env_ok"] == 0


def test_wave_uniform_scalars_must_agree(ask):
    a = shipped("dc_config.json")
    b = shipped("dc_config_r16.json")
    assert all(bits(a[s]) == bits(b[s]) for s in UNIFORM)
    for key in UNIFORM:      # one bit of one wave-uniform scalar: the batch does not qualify (the envs' rows do not mind)
        t = parse_tables(ask(["Z 2", derive_line(0, a), derive_line(1, dict(b, **{key: one_bit_up(b[key])})), "B 2 1 0 1"])[3])
        assert t["wide_gen_ok"] == 0 and t["wide"] == [] and t["prm_env_ok"] == 1, key
    for key in sorted(set(SCALARS) - set(UNIFORM)):      # a per-config scalar may differ: it travels in SdcWideCfg or is not read per lane
        q = dict(b, **{key: one_bit_up(b[key])})
        out = ask(["Z 2", derive_line(0, a), derive_line(1, q), "B 2 1 0 1"])
        t = parse_tables(out[3])
        assert t["wide_gen_ok"] == 1 and same_bits(t["wide"][1], want_wide(q, parse_derived(out[2]))), key
    # seventeen configs: more than the kernel stages
    many = ask(["Z 17"] + [derive_line(i, a) for i in range(17)] + ["B 2 1 3 16"])[-1]
    assert parse_tables(many)["wide_gen_ok"] == 0 and parse_tables(many)["prm_env_ok"] == 1
    assert parse_tables(ask(["Z 16"] + [derive_line(i, a) for i in range(16)] + ["B 2 1 3 15"])[-1])["wide_gen_ok"] == 1


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------
def geometry(ask, cases):
    keys = ("lw", "qstride", "rq_max", "sweep_blocks", "qcum_t", "hist_t", "has_feat", "feat_waves", "feat_use_sma", "feat_lds_bytes")
    return [dict(zip(keys, map(int, ln.split()))) for ln in ask([f"G {n} {t} {f}" for n, t, f in cases])]


def test_geometry(ask):
    week, month, last, first_without = geometry(ask, [(4096, 672, 0), (4096, 2880, 0), (4096, 3178, 0), (4096, 3179, 0)])
    assert (week["lw"], week["qstride"], week["has_feat"], week["feat_waves"], week["feat_use_sma"], week["feat_lds_bytes"]) == (690, 704, 1, 4, 1, 50440)
    assert (month["has_feat"], month["feat_waves"], month["feat_use_sma"], month["feat_lds_bytes"]) == (1, 1, 0, 54872)
    assert last["has_feat"] == 1 and first_without["has_feat"] == 0 and last["feat_lds_bytes"] <= 64 * 1024
    small, mid, large = geometry(ask, [(4096, 672, 0), (32768, 672, 0), (262144, 672, 0)])
    assert [g["rq_max"] for g in (small, mid, large)] == [128, 1024, 2047] and [g["sweep_blocks"] for g in (small, mid, large)] == [32, 128, 128]
    # every episode length that keeps feature rows has a launch that fits, by the header's own rule for each shape
    lengths = list(range(1, 3300))
    for T, g in zip(lengths, geometry(ask, [(64, T, 0) for T in lengths])):
        win, sma, tile = 8 * (2 * T + 43), 8 * (T + 22), 4 * 64 * 33
        assert g["lw"] == T + 18 and g["qstride"] == -(-T // 64) * 64 and g["has_feat"] == int(T <= 3178)
        waves = 4 if win + sma + 4 * tile <= 65536 else 1
        sma_in = int(win + sma + waves * tile <= 65536)
        assert (g["feat_waves"], g["feat_use_sma"], g["feat_lds_bytes"]) == (waves, sma_in, win + sma_in * sma + waves * tile)
        assert not g["has_feat"] or g["feat_lds_bytes"] <= 65536


def test_mirrors_at_the_thresholds_of_the_step_paths(ask):
    sizes = sorted(step_paths.KERNEL_OF_BATCH) + [49152]
    for n, g in zip(sizes, geometry(ask, [(n, 64, 0) for n in sizes])):
        lanes = step_paths.KERNEL_OF_BATCH.get(n, "wide") == "wide"
        assert g["qcum_t"] == int(lanes) and g["hist_t"] == int(lanes and n >= 49152), n      # 49088: the largest batch without the ring's mirror
    forced, odd, off = geometry(ask, [(256, 64, step_paths.WIDE), (250, 64, step_paths.WIDE), (256, 64, step_paths.WIDE_OFF)])
    assert (forced["qcum_t"], forced["hist_t"], odd["qcum_t"], off["qcum_t"]) == (1, 0, 0, 0)


# ---- sdc_config --------------------------------------------------------------------------------------------------------------------------
GOOD = dict(n_envs=4, episode_steps=96, hist_cap=10000, queue_max_len=1000, n_locations=1, n_dc_configs=1, env_index_base=0,
            reward_method=(0, 0, 0), policy=(0, 0, 0))
POLICY_TEXT = "sdc_create: policy must be EXTERNAL or DO_NOTHING, RBC for the battery slot, TRIM_AND_RESPOND for the dc slot"
REFUSALS = [
    (dict(n_envs=0), 0, "sdc_create: n_envs must be > 0"), (dict(n_envs=-1), 0, "sdc_create: n_envs must be > 0"),
    (dict(episode_steps=0), 0, "sdc_create: episode_steps must be > 0"),
    (dict(hist_cap=1), 0, "sdc_create: hist_cap must be in [2, 10240]"), (dict(hist_cap=10241), 0, "sdc_create: hist_cap must be in [2, 10240]"),
    (dict(n_locations=0), 0, "sdc_create: need >= 1 location and dc config"), (dict(n_dc_configs=0), 0, "sdc_create: need >= 1 location and dc config"),
    (dict(env_index_base=-1), 0, "sdc_create: env_index_base must be >= 0"),
    (dict(queue_max_len=0), 0, "sdc_create: bad queue_max_len"), (dict(queue_max_len=65536), 0, "sdc_create: bad queue_max_len"),
    (dict(episode_steps=10363), 0, "sdc_create: episode too long for the 32-bit queue prefix sums"),
    (dict(reward_method=(0, 7, 0)), 1, "sdc_create: unknown reward_method"), (dict(reward_method=(-1, 0, 0)), 1, "sdc_create: unknown reward_method"),
    (dict(policy=(2, 0, 0)), 1, POLICY_TEXT), (dict(policy=(0, 2, 0)), 1, POLICY_TEXT), (dict(policy=(0, 0, 3)), 1, POLICY_TEXT),
    (dict(policy=(3, 0, 0)), 1, POLICY_TEXT), (dict(policy=(0, 0, 4)), 1, POLICY_TEXT), (dict(policy=(0, -1, 0)), 1, POLICY_TEXT),
    # precedence: the first check in the list wins; an argument check before a mode check; a reward method before a policy
    (dict(n_envs=0, episode_steps=0), 0, "sdc_create: n_envs must be > 0"),
    (dict(queue_max_len=0, policy=(2, 0, 0)), 0, "sdc_create: bad queue_max_len"),
    (dict(reward_method=(0, 0, 9), policy=(2, 0, 0)), 1, "sdc_create: unknown reward_method"),
]
TAKEN = [dict(), dict(hist_cap=2), dict(hist_cap=10240), dict(queue_max_len=65535), dict(episode_steps=10362), dict(reward_method=(6, 6, 6)),
         dict(policy=(1, 3, 2)), dict(policy=(1, 1, 1)), dict(n_envs=262144, env_index_base=2 ** 31 - 1)]


def test_every_sdc_config_refusal_with_its_text(ask):
    def line(change):
        c = dict(GOOD, **change)
        return " ".join(map(str, ["K"] + [c[k] for k in ("n_envs", "episode_steps", "hist_cap", "queue_max_len", "n_locations", "n_dc_configs",
                                                         "env_index_base")] + list(c["reward_method"]) + list(c["policy"])))
    out = ask([line(ch) for ch, _, _ in REFUSALS] + [line(ch) for ch in TAKEN])
    assert out[:len(REFUSALS)] == [f"{after} | {text}" for _, after, text in REFUSALS]
    assert out[len(REFUSALS):] == ["0 | -"] * len(TAKEN)
