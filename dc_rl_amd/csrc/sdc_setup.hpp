// sdc_setup.hpp -- WHAT THE HOST DERIVES from sdc_config and sdc_dc_params before anything is uploaded: whether a config is taken at all,
// a data-centre config as the kernels see it (reciprocals, rack classes), the tables and facts of a batch of configs, the sizes sdc_create
// allocates by and the features kernel's launch shape.  sdc_capi.hip calls these functions and copies their results to the device: it
// derives nothing itself.
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_host_setup.py holds it to a
// restatement in Python without a GPU; tests/test_gpu_kernel_reach.py, test_gpu_wide_gen.py, test_gpu_production_sizes.py and
// test_gpu_snapshot.py hold every table to the device's results bit for bit).  DESIGN.md section 4.21 has this file as a table.
// The types the derivation fills are defined here and reach the kernels through sdc_device.hpp.
#pragma once

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/sustaindc_hip.h"
#include "sdc_dispatch.hpp"

#define SDC_BLOCK 256
#define SDC_WAVE 64
#define SDC_HIST_PER_THREAD 40  // 10 x float4 per thread -> 10240 ring slots per env
#define SDC_HIST_STRIDE (SDC_BLOCK * SDC_HIST_PER_THREAD)
#define SDC_FEAT_ROW 32      // floats per feature row (128 bytes)
// deferred window re-centring (sdc_device.hpp SdcRefillReq): request slots per set, by batch size
#define SDC_RQ_MIN 128        // (4096 envs and below)
#define SDC_RQ_LIMIT 2047     // (the request index + 1 has 11 bits in the header's stamp)

// ---- the types ----------------------------------------------------------------------------------------------------------------------
#define SDC_MAX_RACK_CLS 8     // rack classes (and groups) the lane-per-env kernel keeps tables for
// (128 dwords: a wavefront holds the table in two registers, dword j in lane j % 64, and reads entries with v_readlane; the
// doubles fill the first 64 dwords, the integers the second)
struct SdcRackClasses {
  double grp_n[SDC_MAX_RACK_CLS], grp_supply[SDC_MAX_RACK_CLS];     // group g: racks of grp_n cpus with supply approach grp_supply
  double cls_full[SDC_MAX_RACK_CLS], cls_idle[SDC_MAX_RACK_CLS];    // class c (of group g: grp_begin[g] <= c < grp_begin[g + 1])
  int n_grp, n_cls;
  int grp_begin[SDC_MAX_RACK_CLS + 1];
  int cls_of_rack[32];                                               // rack slot -> class
  int pad[21];
};
static_assert(sizeof(SdcRackClasses) == 512 && SDC_MAX_RACK_CLS == 8, "two registers of a wavefront hold the table");

// A data-centre parameter set as the kernels see it: the caller's struct plus correctly rounded reciprocals of the
// parameters the step divides by (sdc_derive_dc below), so that those divisions take the 3-instruction form of sdc_div_const.
struct SdcDcDev {
  sdc_dc_params p;
  double rc_n_racks, rc_itfan_ref_v_ratio, rc_rho_air, rc_ctafr, rc_bat_capacity;
  double k_outlet;   // 1.918 / (c_air rho_air 0.526): the constant factor of the rack outlet-temperature rise
  double n_racks_f;  // p.n_racks as a double (the step kernel hands the scalars from p.m_cpu to here round as doubles)
  double ret_sum;    // sum of rack_return over the config's racks (the CRAC return temperature is (this + sum of outlets) / racks)
  // RACK CLASSES (the lane-per-env kernel, sdc_wide.hip: its rack model is a per-lane LOOP, and a rack's power / outlet temperature
  // depend on its four parameters only): the config's DISTINCT (cpus, supply approach, full load, idle) tuples, grouped by their
  // (cpus, supply approach) pair -- what the fan / airflow / inlet part depends on.  The shipped 20-rack config has 7 classes in 2
  // groups.  n_cls == 0: too many racks or classes for the kernel's tables.
  SdcRackClasses rc;
};

// THE LANE-PER-ENV KERNEL'S GENERAL FORM (sdc_wide.hip, template GEN: several configs in one batch, rule-based policies, alternate
// reward functions of the dc / battery agents): every LANE carries its own config.  What differs between the configs of a batch the
// kernel serves -- the rack table and the quantities sized from it and from the location (utils/make_envs_pyenv.py:139-218) -- is one
// SdcWideCfg per config, staged into LDS by every workgroup (LDS-DMA) and read per lane; the scalars of the server / HVAC
// characteristics (CPU and fan curves, air constants, set-point limits) must be the same bits in every config (the reference's
// dc_config_dc{1,2,3}.json differ in their rack lists only) and stay wave-uniform.  59 doubles per config: an ODD number of 8-byte
// words, so lanes of different configs read different LDS banks.
#define SDC_WIDE_MAX_CLS 12    // rack classes per config (the shipped 20 / 16 / 25-rack configs: 7 / 8 / 11)
#define SDC_WIDE_MAX_CFG 16
enum { WC_RET_SUM = 0, WC_RC_N_RACKS, WC_CT_FAN_REF_P, WC_RC_CTAFR, WC_BAT_CAP, WC_RC_BAT_CAP, WC_SCAL_COUNT };
struct SdcWideCfg {
  double cls[SDC_WIDE_MAX_CLS][4];     // class c: {cpus, supply approach, full load, idle} (unused classes: zeros)
  double scal[WC_SCAL_COUNT];          // the per-config scalars, WC_*
  unsigned map[4];                     // rack slot r -> class: 4 bits each, slot r in bits 4 (r % 8) of map[r / 8]
  int n_cls, n_racks;
  double pad[2];
};
static_assert(sizeof(SdcWideCfg) == 59 * 8, "an odd number of 8-byte words per config");
#define SDC_WIDE_CFG_DOUBLES 59

// ---- sdc_config: refused, or taken -------------------------------------------------------------------------------------------------
// Every check sdc_create makes of its sdc_config, in the order a caller meets them.  `after_device`: the refusal waits behind the
// device's own checks (is there such a device, is it a gfx950), as it always has.
struct SdcRefusal {
  const char* msg;      // nullptr: taken
  bool after_device;
};
inline SdcRefusal sdc_check_config(const sdc_config& c) {
  if (c.n_envs <= 0) return {"sdc_create: n_envs must be > 0", false};
  if (c.episode_steps <= 0) return {"sdc_create: episode_steps must be > 0", false};
  static_assert(SDC_HIST_STRIDE == 10240, "the message below");
  if (c.hist_cap < 2 || c.hist_cap > SDC_HIST_STRIDE) return {"sdc_create: hist_cap must be in [2, 10240]", false};
  if (c.n_locations <= 0 || c.n_dc_configs <= 0) return {"sdc_create: need >= 1 location and dc config", false};
  if (c.env_index_base < 0) return {"sdc_create: env_index_base must be >= 0", false};
  if (c.queue_max_len <= 0 || c.queue_max_len > 65535) return {"sdc_create: bad queue_max_len", false};
  if ((long long)c.episode_steps * 20 > 0x7FFFFFFFLL / c.episode_steps)
    return {"sdc_create: episode too long for the 32-bit queue prefix sums", false};
  for (int a = 0; a < 3; a++)
    if (c.reward_method[a] < 0 || c.reward_method[a] > SDC_REWARD_WATER) return {"sdc_create: unknown reward_method", true};
  for (int a = 0; a < 3; a++) {
    const int pol = c.policy[a];
    if (pol != SDC_POLICY_EXTERNAL && pol != SDC_POLICY_DO_NOTHING && !(a == 2 && pol == SDC_POLICY_RBC) &&
        !(a == 1 && pol == SDC_POLICY_TRIM_AND_RESPOND))
      return {"sdc_create: policy must be EXTERNAL or DO_NOTHING, RBC for the battery slot, TRIM_AND_RESPOND for the dc slot", true};
  }
  return {nullptr, false};
}

// ---- geometry: what sdc_create allocates by and launch_features launches by ----------------------------------------------------------
struct SdcGeometry {
  int lw;                    // weather window: samples per env (the episode + the observations' look-ahead)
  int qstride;               // queue-table slots per env: episode_steps rounded up to 64
  int rq_max, sweep_blocks;  // deferred re-centring: request slots per set; four-wavefront sweep workgroups of a single-step launch
  SdcWideMirrors mirrors;    // which slot-major mirrors the batch gets (sdc_dispatch.hpp)
  // the episode's feature rows (sdc_features.hip): kept iff the kernel's two LDS windows of an env fit in 50 KB; its launch then has
  // feat_waves wavefronts per workgroup, a tile each, beside the windows, and the moving averages in LDS too where they fit (feat_use_sma)
  bool has_feat;
  int feat_waves, feat_use_sma;
  size_t feat_lds_bytes;
};
constexpr size_t SDC_LDS_BYTES = 64 * 1024;                                          // a workgroup's LDS limit
constexpr size_t SDC_FEAT_WIN_MAX_BYTES = 50 * 1024;                                 // feature rows: the windows may take this much ...
constexpr size_t SDC_FEAT_TILE_BYTES = sizeof(float) * SDC_WAVE * (SDC_FEAT_ROW + 1);     // ... beside 8 448 B per wavefront
static_assert(SDC_FEAT_WIN_MAX_BYTES + SDC_FEAT_TILE_BYTES <= SDC_LDS_BYTES, "feature rows imply a launch shape that fits: one wavefront, no moving averages");
inline SdcGeometry sdc_geometry(const sdc_config& c) {
  SdcGeometry g{};
  const int T = c.episode_steps, N = c.n_envs;
  g.lw = T + 18;
  g.qstride = (T + 63) / 64 * 64;
  // ~26 windows per 4096 envs ask per step; a workgroup serves requests b, b + sweep_blocks, ...
  g.rq_max = std::min((int)SDC_RQ_LIMIT, std::max((int)SDC_RQ_MIN, (N / 32 + 127) / 128 * 128));
  g.sweep_blocks = std::min(128, std::max(32, N / 128));
  g.mirrors = sdc_wide_mirrors(N, c.debug_flags);
  const size_t win = sizeof(double) * (size_t)(T + 25 + g.lw), sma = sizeof(double) * (size_t)(T + 22);
  g.has_feat = win <= SDC_FEAT_WIN_MAX_BYTES;      // (longer episodes go without: the step then computes the features itself)
  // four wavefronts share an env's windows (and the windows' moving averages, computed once) where four tiles fit beside them
  g.feat_waves = win + sma + 4 * SDC_FEAT_TILE_BYTES <= SDC_LDS_BYTES ? 4 : 1;
  g.feat_use_sma = win + sma + g.feat_waves * SDC_FEAT_TILE_BYTES <= SDC_LDS_BYTES ? 1 : 0;
  g.feat_lds_bytes = win + (g.feat_use_sma ? sma : 0) + g.feat_waves * SDC_FEAT_TILE_BYTES;
  assert(!g.has_feat || g.feat_lds_bytes <= SDC_LDS_BYTES);
  return g;
}

// ---- one config: sdc_dc_params -> SdcDcDev -------------------------------------------------------------------------------------------
// the DISTINCT (cpus, supply approach, full load, idle) tuples of a config's racks in order of first appearance, and each rack's
// tuple.  Both class tables below start here: the order decides the fp64 summation order of the lane-per-env kernel.  (n_racks <= 32)
struct SdcRackTuples {
  int n;
  double cls[32][4];
  int of_rack[32];
};
inline SdcRackTuples sdc_rack_tuples(const sdc_dc_params& p) {
  SdcRackTuples t{};
  for (int r = 0; r < p.n_racks; r++) {
    const double c[4] = {p.rack_n[r], p.rack_supply[r], p.rack_full[r], p.rack_idle[r]};
    int k = 0;
    while (k < t.n && !(t.cls[k][0] == c[0] && t.cls[k][1] == c[1] && t.cls[k][2] == c[2] && t.cls[k][3] == c[3])) k++;
    if (k == t.n) std::memcpy(t.cls[t.n++], c, sizeof(c));
    t.of_rack[r] = k;
  }
  return t;
}
// SdcRackClasses: up to 32 racks in up to SDC_MAX_RACK_CLS classes (else n_cls == 0, every field zero), the classes renumbered group by
// group -- groups keyed (cpus, supply approach), in order of first appearance, a group's classes likewise
inline SdcRackClasses sdc_rack_classes(const sdc_dc_params& p) {
  SdcRackClasses rc{};
  if (p.n_racks > 32) return rc;
  const SdcRackTuples t = sdc_rack_tuples(p);
  if (t.n > SDC_MAX_RACK_CLS) return rc;
  int grp_of[SDC_MAX_RACK_CLS], renum[SDC_MAX_RACK_CLS];
  for (int j = 0; j < t.n; j++) {
    int g = 0;
    while (g < rc.n_grp && !(rc.grp_n[g] == t.cls[j][0] && rc.grp_supply[g] == t.cls[j][1])) g++;
    if (g == rc.n_grp) {
      rc.grp_n[g] = t.cls[j][0];
      rc.grp_supply[g] = t.cls[j][1];
      rc.n_grp++;
    }
    grp_of[j] = g;
  }
  for (int g = 0; g < rc.n_grp; g++) {
    rc.grp_begin[g] = rc.n_cls;
    for (int j = 0; j < t.n; j++)
      if (grp_of[j] == g) {
        renum[j] = rc.n_cls;
        rc.cls_full[rc.n_cls] = t.cls[j][2];
        rc.cls_idle[rc.n_cls] = t.cls[j][3];
        rc.n_cls++;
      }
  }
  rc.grp_begin[rc.n_grp] = rc.n_cls;
  for (int r = 0; r < p.n_racks; r++) rc.cls_of_rack[r] = renum[t.of_rack[r]];
  return rc;
}
// SdcWideCfg: up to 32 racks in up to SDC_WIDE_MAX_CLS classes (else false), the classes in order of first appearance
inline bool sdc_wide_cfg_of(const SdcDcDev& e, SdcWideCfg& w) {
  w = SdcWideCfg{};
  if (e.p.n_racks > 32) return false;
  const SdcRackTuples t = sdc_rack_tuples(e.p);
  if (t.n > SDC_WIDE_MAX_CLS) return false;
  std::memcpy(w.cls, t.cls, sizeof(double) * 4 * (size_t)t.n);
  for (int r = 0; r < e.p.n_racks; r++) w.map[r >> 3] |= (unsigned)t.of_rack[r] << (4 * (r & 7));
  w.n_cls = t.n;
  w.n_racks = e.p.n_racks;
  w.scal[WC_RET_SUM] = e.ret_sum; w.scal[WC_RC_N_RACKS] = e.rc_n_racks; w.scal[WC_CT_FAN_REF_P] = e.p.ct_fan_ref_p;
  w.scal[WC_RC_CTAFR] = e.rc_ctafr; w.scal[WC_BAT_CAP] = e.p.bat_capacity_mwh; w.scal[WC_RC_BAT_CAP] = e.rc_bat_capacity;
  return true;
}

// a divisor the kernels' 3-instruction division (sdc_div_const) is exact for: positive, finite, its significand not all ones
inline bool sdc_divisor_ok(const double x) {
  unsigned long long bits;
  std::memcpy(&bits, &x, 8);
  return x > 0 && std::isfinite(x) && (bits & 0xFFFFFFFFFFFFFull) != 0xFFFFFFFFFFFFFull;
}
// sdc_set_dc_params: -> nullptr and `e` filled, or the reason the config is refused
inline const char* sdc_derive_dc(const sdc_dc_params& p, SdcDcDev& e) {
  if (p.n_racks <= 0 || p.n_racks > SDC_MAX_RACKS) return "sdc_set_dc_params: n_racks must be in [1, 64]";
  e = SdcDcDev{};
  e.p = p;
  const double divisors[5] = {(double)p.n_racks, p.itfan_ref_v_ratio, p.rho_air, p.ctafr, p.bat_capacity_mwh};
  double* const rcs[5] = {&e.rc_n_racks, &e.rc_itfan_ref_v_ratio, &e.rc_rho_air, &e.rc_ctafr, &e.rc_bat_capacity};
  for (int i = 0; i < 5; i++) {
    if (!sdc_divisor_ok(divisors[i]))
      return "sdc_set_dc_params: n_racks, itfan_ref_v_ratio, rho_air, ctafr and bat_capacity_mwh must be "
             "positive, finite, and not have an all-ones significand";
    *rcs[i] = 1.0 / divisors[i];
  }
  e.k_outlet = 1.918 / (p.c_air * p.rho_air * 0.526);
  e.n_racks_f = (double)p.n_racks;
  for (int r = 0; r < p.n_racks; r++) e.ret_sum += p.rack_return[r];
  e.rc = sdc_rack_classes(p);
  return nullptr;
}

// ---- a batch of configs: the facts sdc_dispatch.hpp asks for, and the tables behind them ----------------------------------------------
struct SdcConfigFacts {
  int racks_cfg0 = 0;         // racks of config 0 (0: not set; the specialised kernels take <= 32: one pass) ...
  int rack_cls_cfg0 = 0;      // ... and its rack classes (SdcRackClasses; 0: more than the lane-per-env kernel's tables hold)
  bool prm_env_ok = false;    // several configs, all set, the envs assigned: every env has its own copy of its config's scalars ...
  int racks_max = 0;          // ... and this is the largest rack count in use
  bool wide_gen_ok = false;   // every config is set and qualifies for the lane-per-env kernel's general form (SdcWideCfg)
};
// a config's scalars lie contiguously from sdc_dc_params::m_cpu to SdcDcDev::ret_sum (sdc_step.hip's P_* enum, asserted there): a row
// of the two scalar tables below
constexpr size_t SDC_PRM_ROW = 32;
constexpr size_t P_COUNT_HOST = (offsetof(SdcDcDev, ret_sum) - offsetof(SdcDcDev, p.m_cpu)) / sizeof(double) + 1;
static_assert(P_COUNT_HOST <= SDC_PRM_ROW, "prm_env rows are 32 doubles");
// the scalars the lane-per-env kernel's general form keeps WAVE-UNIFORM (read from config 0): the same bits in every config, or the
// batch does not qualify
constexpr size_t SDC_WAVE_UNIFORM[] = {
    offsetof(SdcDcDev, p.m_cpu), offsetof(SdcDcDev, p.c_cpu), offsetof(SdcDcDev, p.rs_cpu), offsetof(SdcDcDev, p.m_fan),
    offsetof(SdcDcDev, p.c_fan), offsetof(SdcDcDev, p.rs_fan), offsetof(SdcDcDev, p.itfan_ref_p), offsetof(SdcDcDev, p.itfan_ref_v_ratio),
    offsetof(SdcDcDev, p.it_fan_full_load_v), offsetof(SdcDcDev, p.c_air), offsetof(SdcDcDev, p.rho_air), offsetof(SdcDcDev, p.crac_supply_pu),
    offsetof(SdcDcDev, p.min_temp), offsetof(SdcDcDev, p.max_temp), offsetof(SdcDcDev, rc_itfan_ref_v_ratio), offsetof(SdcDcDev, rc_rho_air),
    offsetof(SdcDcDev, k_outlet)};
inline bool sdc_wave_uniform_same(const SdcDcDev& a, const SdcDcDev& b) {
  for (const size_t off : SDC_WAVE_UNIFORM)
    if (std::memcmp(reinterpret_cast<const char*>(&a) + off, reinterpret_cast<const char*>(&b) + off, sizeof(double)) != 0) return false;
  return true;
}
// the largest rack count among the configs the envs are assigned to (what a clone or restore, which moves assignments, refreshes)
inline int sdc_racks_max(const SdcDcDev* dc, const int* cfg_of_env, const int n_envs) {
  int most = 0;
  for (int e = 0; e < n_envs; e++) most = std::max(most, dc[cfg_of_env[e]].p.n_racks);
  return most;
}

struct SdcConfigTables {
  SdcConfigFacts facts;
  std::vector<double> prm_env, prm_cfg;     // prm_env_ok: [n_envs][32] every env's copy of its config's scalars; [n_cfg][32] the same by config
  std::vector<SdcWideCfg> wide;             // wide_gen_ok: [n_cfg] ...
  int wide_max_cls = 0, wide_max_racks4 = 0;      // ... the largest class count of a config; the largest rack count rounded up to four
};
// dc[c] is config c where set[c], zeros where it has not been set yet; cfg_of_env: [n_envs], or nullptr before the first assignment
inline SdcConfigTables sdc_config_tables(const SdcDcDev* dc, const unsigned char* set, const int n_cfg, const int* cfg_of_env,
                                         const int n_envs) {
  SdcConfigTables t;
  SdcConfigFacts& f = t.facts;
  if (set[0]) {
    f.racks_cfg0 = dc[0].p.n_racks;
    f.rack_cls_cfg0 = dc[0].rc.n_cls;
  }
  const bool all_set = std::all_of(set, set + n_cfg, [](const unsigned char s) { return s != 0; });
  if (!all_set) return t;
  if (n_cfg > 1 && cfg_of_env) {
    const auto row = [](std::vector<double>& tab, const size_t i, const SdcDcDev& e) {
      std::memcpy(&tab[i * SDC_PRM_ROW], &e.p.m_cpu, sizeof(double) * P_COUNT_HOST);
    };
    t.prm_env.assign((size_t)n_envs * SDC_PRM_ROW, 0.0);
    for (int e = 0; e < n_envs; e++) row(t.prm_env, (size_t)e, dc[cfg_of_env[e]]);
    t.prm_cfg.assign((size_t)n_cfg * SDC_PRM_ROW, 0.0);
    for (int c = 0; c < n_cfg; c++) row(t.prm_cfg, (size_t)c, dc[c]);
    f.racks_max = sdc_racks_max(dc, cfg_of_env, n_envs);
    f.prm_env_ok = true;
  }
  if (n_cfg > SDC_WIDE_MAX_CFG) return t;
  t.wide.resize((size_t)n_cfg);
  int max_racks = 0;
  for (int c = 0; c < n_cfg; c++) {
    if (!sdc_wave_uniform_same(dc[c], dc[0]) || !sdc_wide_cfg_of(dc[c], t.wide[(size_t)c])) {
      t.wide.clear();
      t.wide_max_cls = 0;
      return t;
    }
    t.wide_max_cls = std::max(t.wide_max_cls, t.wide[(size_t)c].n_cls);
    max_racks = std::max(max_racks, dc[c].p.n_racks);
  }
  t.wide_max_racks4 = (max_racks + 3) / 4 * 4;
  f.wide_gen_ok = true;
  return t;
}
