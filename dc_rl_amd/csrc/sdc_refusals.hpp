// sdc_refusals.hpp -- WHAT THE C-ABI REFUSES, AND WITH WHICH WORDS: every refusal of an entry point that can be decided without a HIP
// call, as one pure function per entry point -- what the library knows of the handle (SdcCallFacts) and the call's arguments in, the
// message out, nothing else.  The texts, and the order in which two faults in one call are reported, are part of the interface.
//
// Plain C++17: no HIP, no sdc_handle, no error string, no return code, no device pointer followed -- a host compiler alone builds it
// (tests/test_host_refusals.py runs the table of tests/refusal_cases.py through it without a GPU, plain and under the sanitizers;
// tests/test_gpu_refusal_wiring.py holds the library to the same literals).  sdc_capi.hip fills the facts (call_facts), asks the
// entry point's rule and turns a message into -2 with sdc_last_error set.  DESIGN.md section 4.25.
//
// A rule's answer: rules whose texts are all fixed return const char* (nullptr: accepted); the others return SdcMsg (no value:
// accepted) and build their string on the refusing path alone.  Caller arrays on the host (env lists, manifests, the overrides' days
// and hours, parameter structs) are read; output arrays and device arrays are looked at as addresses only.  By-products (the
// objective with its defaults filled in, an inverse index map, the validated copies of sdc_plan_terms / sdc_plan_forecast) are
// out-parameters, written on acceptance.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "../../include/sustaindc_hip.h"
#include "sdc_critic_pack.hpp"
#include "sdc_dispatch.hpp"
#include "sdc_mirror.hpp"
#include "sdc_mpc_schedule.hpp"
#include "sdc_optim.hpp"
#include "sdc_minibatch.hpp"

using SdcMsg = std::optional<std::string>;

// ---- what a refusal may know of a handle ------------------------------------------------------------------------------------------------
// sdc_capi.hip's call_facts fills it.  A constant that only a HIP header defines arrives here as a field.  The part that sdc_step,
// sdc_rollout and sdc_rollout_actor read is a struct of its own, so that a step builds these few scalars and nothing else
// (stepping_facts; measured: with the whole struct built per step the headline rate fell by 0.4 %).
struct SdcSteppingFacts {
  bool handle = false;                 // false: the handle was NULL, and nothing else here means anything
  bool started = false;                // a reset has been made
  int left = 0;                        // steps to the end of the episode that ends first (the mirror's steps_to_terminal)
  int debug_flags = 0;                 // sdc_config's
  bool all_policies = false;           // every agent slot has a policy (actions may be NULL)
  bool actor_set[3] = {false, false, false};
  int actor_activation[3] = {0, 0, 0};
  bool latch_valid = false;            // the library's copy of the latest observations is current
  bool critic_set = false;
};
struct SdcCallFacts : SdcSteppingFacts {
  int n_envs = 0, episode_steps = 0, hist_cap = 0, n_locations = 0, n_dc_configs = 0, auto_reset = 0;      // sdc_config's
  bool tables_set = false, assigned = false;
  bool has_feat = false;               // the engine keeps feature rows at all
  uint32_t state_layout = 0;           // sdc_state_layout()
  int qstride = 0, lw = 0;             // sdc_queue_stride(), sdc_weather_window_len()
  int rec_dwords = 0, rec_cfg = 0;     // dwords of an env's state record, and which of them holds its config id
  int mark_engine_id = 0;              // this handle's id in mark manifests (0: it has taken no mark)
  sdc_plan_forecast forecast{};        // sdc_set_plan_forecast's
  const SdcHostMirror* mirror = nullptr;
  SdcStepFacts step{};                 // sdc_rollout_actor_stats' closed-loop rule: what step_facts() builds for the call
};

// the addresses OR-ed together: one test of the low bits for a rule about several arrays
template <class... P>
static inline uintptr_t sdc_addr_bits(const P*... p) {
  return (uintptr_t{0} | ... | reinterpret_cast<uintptr_t>(p));
}

// ---- stepping and setup -------------------------------------------------------------------------------------------------------------------
static inline const char* sdc_set_tables_refused(const SdcCallFacts& f, const int loc_id, const double* W, const double* C, const double* T,
                                          const double* WB, const int n) {
  if (!f.handle || !W || !C || !T || !WB) return "sdc_set_tables: null argument";
  if (loc_id < 0 || loc_id >= f.n_locations) return "sdc_set_tables: loc_id out of range";
  static_assert(SDC_TABLE_LEN == 35040, "the message below");
  if (n != SDC_TABLE_LEN) return "sdc_set_tables: tables must hold 35040 samples";
  return nullptr;
}

// (what the parameters themselves are refused for: sdc_setup.hpp sdc_derive_dc)
static inline const char* sdc_set_dc_params_refused(const SdcCallFacts& f, const int cfg_id, const sdc_dc_params* p) {
  if (!f.handle || !p) return "sdc_set_dc_params: null argument";
  if (cfg_id < 0 || cfg_id >= f.n_dc_configs) return "sdc_set_dc_params: cfg_id out of range";
  return nullptr;
}

static inline const char* sdc_assign_envs_refused(const SdcCallFacts& f, const int32_t* loc_id, const int32_t* cfg_id, const int32_t* day_lo,
                                           const int32_t* day_hi) {
  if (!f.handle || !loc_id || !cfg_id || !day_lo || !day_hi) return "sdc_assign_envs: null argument";
  for (int e = 0; e < f.n_envs; e++) {
    if (loc_id[e] < 0 || loc_id[e] >= f.n_locations) return "sdc_assign_envs: loc_id out of range";
    if (cfg_id[e] < 0 || cfg_id[e] >= f.n_dc_configs) return "sdc_assign_envs: cfg_id out of range";
    if (day_lo[e] < 0 || day_hi[e] > 364 || day_lo[e] > day_hi[e]) return "sdc_assign_envs: bad day range";
  }
  return nullptr;
}

// mask: [N] or NULL (the whole batch); the overrides' ranges are checked for the envs that are reset
static inline const char* sdc_reset_refused(const SdcCallFacts& f, const uint8_t* mask, const sdc_reset_override* ovr) {
  if (!f.handle) return "sdc_reset: null handle";
  if (!f.tables_set || !f.assigned) return "sdc_reset: call sdc_set_tables / sdc_set_dc_params / sdc_assign_envs first";
  if (ovr && ovr->noise) {
    if (!ovr->day || !ovr->hour || !ovr->roll_days) return "sdc_reset: noise injection needs day, hour and roll_days";
    for (int e = 0; e < f.n_envs; e++) {
      if (mask && !mask[e]) continue;
      if (ovr->day[e] < 0 || ovr->day[e] > 364 || ovr->hour[e] < 0 || ovr->hour[e] > 23 || ovr->roll_days[e] < 0 || ovr->roll_days[e] > 364)
        return "sdc_reset: injected day / hour / roll_days out of range";
    }
  } else if (ovr) {
    if (!ovr->day || !ovr->hour || !ovr->ci_min || !ovr->ci_max || !ovr->t_min || !ovr->t_max || !ovr->t_win || !ovr->wb_win)
      return "sdc_reset: incomplete override";
    for (int e = 0; e < f.n_envs; e++) {
      if (mask && !mask[e]) continue;
      if (ovr->day[e] < 0 || ovr->day[e] > 364 || ovr->hour[e] < 0 || ovr->hour[e] > 23) return "sdc_reset: override day/hour out of range";
    }
  }
  return nullptr;
}

// info: optional (NULL: not wanted) -- but for verify mode, whose kernel reads info[energy_z] and raises its fault bit there.  (A caller of
// this rule that does not say has said NULL: the refusing side.)
static inline const char* sdc_step_refused(const SdcSteppingFacts& f, const int32_t* actions, const float* obs, const float* rew, const uint8_t* done,
                                           const float* info = nullptr) {
  if (!f.handle || !obs || !rew || !done) return "sdc_step: null argument";
  if (!actions && !f.all_policies) return "sdc_step: actions may only be NULL when every agent slot has a policy";
  if (!f.started) return "sdc_step: sdc_reset must be called first";
  if (f.left <= 0) return "sdc_step: an environment has finished its episode; call sdc_reset (auto_reset is off)";
  if ((f.debug_flags & SDC_DEBUG_VERIFY) && !info) return "sdc_step: verify mode reports through info; info may not be NULL";
  return nullptr;
}

// the two multi-step calls' words for a launch that would cross an episode's end
static inline std::string sdc_rollout_past_end(const char* who, const int left) {
  return std::string(who) + ": the rollout would run past the end of an episode (" + std::to_string(left) + " steps left); split it there";
}

static inline SdcMsg sdc_rollout_refused(const SdcSteppingFacts& f, const int n_steps, const int32_t* actions, const float* obs, const float* rew,
                                  const uint8_t* done) {
  if (!f.handle || !obs || !rew || !done) return "sdc_rollout: null argument";
  if (!actions && !f.all_policies) return "sdc_rollout: actions may only be NULL when every agent slot has a policy";
  if (!f.started) return "sdc_rollout: sdc_reset must be called first";
  if (n_steps <= 0) return "sdc_rollout: n_steps must be positive";
  if (n_steps > f.left) return sdc_rollout_past_end("sdc_rollout", f.left);
  if (f.debug_flags & SDC_DEBUG_VERIFY) return "sdc_rollout: verify mode checks single steps; use sdc_step";
  return std::nullopt;
}

static inline const char* sdc_set_actor_refused(const SdcCallFacts& f, const int slot, const sdc_actor_params* p) {
  if (!f.handle || !p) return "sdc_set_actor: null argument";
  if (slot < 0 || slot > 2) return "sdc_set_actor: agent_slot must be 0 (ls), 1 (dc) or 2 (bat)";
  if (p->activation < 0 || p->activation > 1) return "sdc_set_actor: activation must be 0 (tanh) or 1 (relu)";
  return nullptr;
}

// what the closed loop asks of the actors and the batch, in the words sdc_rollout_actor and sdc_rollout_actor_stats share (behind
// their "who: ")
constexpr const char* SDC_ACTORS_NOT_SET = "sdc_set_actor all three agents first";
constexpr const char* SDC_ACTORS_ACTIVATION =
    "the three actors must share one activation (the reference builds them from one model config: happo.yaml activation_func)";
constexpr const char* SDC_ACTORS_NO_OBS = "no observations yet (the actors were set after the last reset / step: reset or step once)";
constexpr const char* SDC_ACTORS_COMMON_CASE =
    "needs the common case (lock-step batch with feature rows, one data-centre config of <= 32 racks, external-action slots, default "
    "rewards, an even number of envs, no debug flags)";
static inline bool sdc_actors_all_set(const SdcSteppingFacts& f) { return f.actor_set[0] && f.actor_set[1] && f.actor_set[2]; }
static inline bool sdc_actors_one_activation(const SdcSteppingFacts& f) {
  return f.actor_activation[0] == f.actor_activation[1] && f.actor_activation[0] == f.actor_activation[2];
}

// (step: step_facts of the call's own arrays, the actions the actors')
static inline SdcMsg sdc_rollout_actor_refused(const SdcSteppingFacts& f, const SdcStepFacts& step, const int n_steps, const float* obs, const float* share_obs, const float* rew,
                                        const uint8_t* done, const float* info, const int32_t* actions_out) {
  const auto w = [](const char* text) { return std::string("sdc_rollout_actor: ") + text; };      // (the refusing path's)
  if (!f.handle || !obs || !share_obs || !rew || !done || !info || !actions_out) return "sdc_rollout_actor: null argument";
  if (!sdc_actors_all_set(f)) return w(SDC_ACTORS_NOT_SET);
  if (!sdc_actors_one_activation(f)) return w(SDC_ACTORS_ACTIVATION);
  if (!f.started) return "sdc_rollout_actor: sdc_reset must be called first";
  if (!f.latch_valid) return w(SDC_ACTORS_NO_OBS);
  if (n_steps <= 0) return "sdc_rollout_actor: n_steps must be positive";
  if (n_steps > f.left) return sdc_rollout_past_end("sdc_rollout_actor", f.left);
  if (sdc_actor_path(step).refused) return w(SDC_ACTORS_COMMON_CASE);
  return std::nullopt;
}

static inline const char* sdc_profile_enable_refused(const SdcSteppingFacts& f) { return f.handle ? nullptr : "sdc_profile_enable: null handle"; }
static inline const char* sdc_profile_read_refused(const SdcSteppingFacts& f, const double* out5) {
  return !f.handle || !out5 ? "sdc_profile_read: null argument" : nullptr;
}

// a named field of sdc_get_state / sdc_set_state as sdc_capi.hip's table has it (NULL: no field of that name)
struct SdcFieldFacts {
  size_t elem;        // bytes per env
  bool allocated;     // false: an array this batch does not have (the slot-major mirrors of a small batch)
};
static inline SdcMsg sdc_get_state_refused(const SdcCallFacts& f, const char* field, const void* host_buf, const size_t bytes,
                                    const SdcFieldFacts* fld) {
  if (!f.handle || !field || !host_buf) return "sdc_get_state: null argument";
  if (!fld) return std::string("sdc_get_state: unknown field ") + field;
  if (bytes != fld->elem * (size_t)f.n_envs) return std::string("sdc_get_state: size mismatch for ") + field;
  if (!fld->allocated) return std::string("sdc_get_state: this batch has no ") + field;
  return std::nullopt;
}
// what the kernels index with is refused BEFORE anything reaches the device: a config id out of range would index the configs / the
// per-env config scalars out of bounds on the next step
static inline SdcMsg sdc_set_state_refused(const SdcCallFacts& f, const char* field, const void* host_buf, const size_t bytes,
                                    const SdcFieldFacts* fld) {
  if (!f.handle || !field || !host_buf) return "sdc_set_state: null argument";
  if (!fld) return std::string("sdc_set_state: unknown field ") + field;
  if (std::strcmp(field, "qcum_t") == 0 || std::strcmp(field, "hist_t") == 0)
    return std::string("sdc_set_state: ") + field + " is derived from " + (field[0] == 'q' ? "qtab" : "hist") + ": write that";
  if (bytes != fld->elem * (size_t)f.n_envs) return std::string("sdc_set_state: size mismatch for ") + field;
  const bool is_cfg = std::strcmp(field, "cfg_id") == 0, is_record = std::strcmp(field, "record") == 0;
  if (is_cfg || is_record) {
    const int32_t* c = static_cast<const int32_t*>(host_buf);
    for (int e = 0; e < f.n_envs; e++) {
      const int id = is_cfg ? c[e] : c[(size_t)e * (size_t)f.rec_dwords + (size_t)f.rec_cfg];
      if (id < 0 || id >= f.n_dc_configs)
        return is_cfg ? "sdc_set_state: cfg_id out of range" : "sdc_set_state: record with a cfg_id out of range";
    }
  }
  return std::nullopt;
}

// ---- the env-copy calls (clone, snapshot / restore, mark / rewind) -----------------------------------------------------------------------
// The inverse map of n entries (envs[k], vals ? vals[k] : k) -- map[env] = its value, -1 for the other envs -- or why the entries have
// none ("" if they have), without the caller's prefix: an env outside [0, N); a value outside [0, n_vals) (n_vals > 0, `val_noun`:
// checked entry by entry with the env); an env that appears twice (`twice`: the caller's noun for it).  map == nullptr: the ranges only
static inline std::string sdc_unique_index_map(const int32_t* envs, const int32_t* vals, const int n, const int N, const int n_vals,
                                        const char* val_noun, const char* twice, std::vector<int>* map) {
  const auto outside = [](const char* noun, const int v, const int k, const int bound) {
    return std::string(noun) + " " + std::to_string(v) + " (entry " + std::to_string(k) + ") outside [0, " + std::to_string(bound) + ")";
  };
  for (int k = 0; k < n; k++) {
    if (envs[k] < 0 || envs[k] >= N) return outside("env", envs[k], k, N);
    if (n_vals > 0 && (vals[k] < 0 || vals[k] >= n_vals)) return outside(val_noun, vals[k], k, n_vals);
  }
  if (!map) return "";
  map->assign((size_t)N, -1);
  for (int k = 0; k < n; k++) {
    if ((*map)[(size_t)envs[k]] >= 0) return std::string(twice) + " " + std::to_string(envs[k]) + " appears twice";
    (*map)[(size_t)envs[k]] = vals ? vals[k] : k;
  }
  return "";
}
// the caller's row buffer (snapshot rows, mark rows): nullptr if it may be used, else why not
static inline const char* sdc_rows_error(const void* rows) { return (sdc_addr_bits(rows) & 255u) != 0 ? "rows must be 256-byte aligned" : nullptr; }

// src_of: dst -> its src, -1 for the other envs
static inline SdcMsg sdc_clone_envs_refused(const SdcCallFacts& f, const int32_t* src, const int32_t* dst, const int n, std::vector<int>& src_of) {
  if (!f.handle) return "sdc_clone_envs: null handle";
  if (n <= 0) return "sdc_clone_envs: n must be positive";
  if (!src || !dst) return "sdc_clone_envs: null index array";
  if (!f.started) return "sdc_clone_envs: sdc_reset must be called first";
  const int N = f.n_envs;
  for (int k = 0; k < n; k++)
    if (src[k] < 0 || src[k] >= N || dst[k] < 0 || dst[k] >= N)
      return "sdc_clone_envs: pair " + std::to_string(k) + " (" + std::to_string(src[k]) + " -> " + std::to_string(dst[k]) +
             ") has an env index outside [0, " + std::to_string(N) + ")";
  const std::string why = sdc_unique_index_map(dst, src, n, N, 0, nullptr, "dst", &src_of);
  if (!why.empty()) return "sdc_clone_envs: " + why;
  for (int k = 0; k < n; k++)
    if (src_of[(size_t)src[k]] >= 0) return "sdc_clone_envs: env " + std::to_string(src[k]) + " is both a src and a dst";
  return std::nullopt;
}

// (an env may appear twice: a snapshot only reads)
static inline SdcMsg sdc_snapshot_envs_refused(const SdcCallFacts& f, const int32_t* envs, const int n, const void* rows, const int32_t* manifest,
                                        const float* obs, const float* share_obs) {
  if (!f.handle) return "sdc_snapshot_envs: null handle";
  if (n <= 0) return "sdc_snapshot_envs: n must be positive";
  if (!envs || !rows || !manifest || !obs || !share_obs) return "sdc_snapshot_envs: null array";
  if (!f.started) return "sdc_snapshot_envs: sdc_reset must be called first";
  const int N = f.n_envs;
  if (n > N) return "sdc_snapshot_envs: n = " + std::to_string(n) + " is more than the batch's " + std::to_string(N) + " envs";
  const std::string why = sdc_unique_index_map(envs, nullptr, n, N, 0, nullptr, nullptr, nullptr);
  if (!why.empty()) return "sdc_snapshot_envs: " + why;
  if (const char* w = sdc_rows_error(rows)) return std::string("sdc_snapshot_envs: ") + w;
  return std::nullopt;
}

// why a manifest row cannot be restored into this engine ("" if it can)
static inline std::string sdc_snap_manifest_error(const SdcCallFacts& f, const int32_t* m) {
  const int32_t want[5] = {(int32_t)f.state_layout, f.episode_steps, f.hist_cap, f.qstride, f.lw};
  static const char* what[5] = {"state layout", "episode_steps", "hist_cap", "queue stride", "weather window length"};
  static_assert(SDC_SNAP_LAYOUT == 0 && SDC_SNAP_EPISODE_STEPS == 1 && SDC_SNAP_HIST_CAP == 2 && SDC_SNAP_QUEUE_STRIDE == 3 &&
                SDC_SNAP_WINDOW_LEN == 4, "the manifest's shape entries come first");
  for (int i = 0; i < 5; i++)
    if (m[i] != want[i]) return std::string(what[i]) + " " + std::to_string(m[i]) + ", this engine's is " + std::to_string(want[i]);
  if (m[SDC_SNAP_T_REL] < 0 || m[SDC_SNAP_T_REL] > f.episode_steps)
    return "episode step " + std::to_string(m[SDC_SNAP_T_REL]) + " outside [0, episode_steps]";
  if (m[SDC_SNAP_FEAT_OK] != 0 && m[SDC_SNAP_FEAT_OK] != 1) return "feature-rows flag " + std::to_string(m[SDC_SNAP_FEAT_OK]);
  if (m[SDC_SNAP_CFG_ID] < 0 || m[SDC_SNAP_CFG_ID] >= f.n_dc_configs)
    return "cfg_id " + std::to_string(m[SDC_SNAP_CFG_ID]) + ", this engine has " + std::to_string(f.n_dc_configs) + " dc configs";
  if (m[SDC_SNAP_LOC_ID] < 0 || m[SDC_SNAP_LOC_ID] >= f.n_locations)
    return "loc_id " + std::to_string(m[SDC_SNAP_LOC_ID]) + ", this engine has " + std::to_string(f.n_locations) + " locations";
  return "";
}

// row_of: dst env -> its row, -1 for the other envs
static inline SdcMsg sdc_restore_envs_refused(const SdcCallFacts& f, const int32_t* rows_idx, const int32_t* envs, const int n, const void* rows,
                                       const int n_rows, const int32_t* manifest, const float* obs, const float* share_obs,
                                       std::vector<int>& row_of) {
  if (!f.handle) return "sdc_restore_envs: null handle";
  if (n <= 0) return "sdc_restore_envs: n must be positive";
  if (n_rows <= 0) return "sdc_restore_envs: n_rows must be positive";
  if (!rows_idx || !envs || !rows || !manifest || !obs || !share_obs) return "sdc_restore_envs: null array";
  if (!f.started) return "sdc_restore_envs: sdc_reset must be called first";
  const std::string bad = sdc_unique_index_map(envs, rows_idx, n, f.n_envs, n_rows, "row", "dst", &row_of);
  if (!bad.empty()) return "sdc_restore_envs: " + bad;
  for (int k = 0; k < n; k++) {
    const std::string why = sdc_snap_manifest_error(f, manifest + (size_t)rows_idx[k] * SDC_SNAPSHOT_MANIFEST);
    if (!why.empty()) return "sdc_restore_envs: row " + std::to_string(rows_idx[k]) + ": " + why;
  }
  if (const char* w = sdc_rows_error(rows)) return std::string("sdc_restore_envs: ") + w;
  return std::nullopt;
}

// the arguments sdc_mark_envs and sdc_rewind_envs refuse alike ("" if they pass)
static inline std::string sdc_mark_args_error(const SdcCallFacts& f, const int32_t* envs, const int n, const void* rows, const void* manifest,
                                       const void* obs, const void* share_obs) {
  if (n <= 0) return "n must be positive";
  if (!rows || !manifest || !obs || !share_obs) return "null array";
  if (!f.started) return "sdc_reset must be called first";
  const int N = f.n_envs;
  if (n > N) return "n = " + std::to_string(n) + " is more than the batch's " + std::to_string(N) + " envs";
  if (!envs && n != N) return "envs == NULL means the whole batch: n must be " + std::to_string(N) + ", not " + std::to_string(n);
  if (envs) {
    const std::string why = sdc_unique_index_map(envs, nullptr, n, N, 0, nullptr, nullptr, nullptr);
    if (!why.empty()) return why;
  }
  if (const char* w = sdc_rows_error(rows)) return w;
  return "";
}

// row_of: env -> its row (envs != NULL only)
static inline SdcMsg sdc_mark_envs_refused(const SdcCallFacts& f, const int32_t* envs, const int n, const int max_steps, const void* rows,
                                    const int32_t* manifest, const float* obs, const float* share_obs, std::vector<int>& row_of) {
  if (!f.handle) return "sdc_mark_envs: null handle";
  if (max_steps < 1 || max_steps > SDC_MARK_MAX_STEPS)
    return "sdc_mark_envs: max_steps = " + std::to_string(max_steps) + " outside [1, " + std::to_string(SDC_MARK_MAX_STEPS) + "]";
  const std::string why = sdc_mark_args_error(f, envs, n, rows, manifest, obs, share_obs);
  if (!why.empty()) return "sdc_mark_envs: " + why;
  if (envs) {
    const std::string twice = sdc_unique_index_map(envs, nullptr, n, f.n_envs, 0, nullptr, "env", &row_of);
    if (!twice.empty()) return "sdc_mark_envs: " + twice;
  }
  return std::nullopt;
}

// row_of as above; overrun: the envs whose mark has been overrun (more steps taken than it reaches) -- the scan goes on behind the first
// refusal, and the caller kills every one of them: slots beyond the row's reach have been overwritten, nothing can bring such a mark back
static inline SdcMsg sdc_rewind_envs_refused(const SdcCallFacts& f, const int32_t* envs, const int n, const void* rows, const int32_t* manifest,
                                      const float* obs, const float* share_obs, std::vector<int>& row_of, std::vector<int>& overrun) {
  if (!f.handle) return "sdc_rewind_envs: null handle";
  std::string why = sdc_mark_args_error(f, envs, n, rows, manifest, obs, share_obs);
  if (!why.empty()) return "sdc_rewind_envs: " + why;
  const SdcHostMirror& mir = *f.mirror;
  const int32_t layout = (int32_t)f.state_layout;
  const int max_steps = manifest[SDC_MARK_M_STEPS];
  if (max_steps < 1 || max_steps > SDC_MARK_MAX_STEPS)
    return "sdc_rewind_envs: manifest with max_steps = " + std::to_string(max_steps) + " outside [1, " + std::to_string(SDC_MARK_MAX_STEPS) +
           "]";
  if (envs) row_of.assign((size_t)f.n_envs, -1);
  int bad_k = -1, bad_why = 0;      // (a message is built for the first refused row only)
  for (int k = 0; k < n; k++) {
    const int e = envs ? envs[k] : k;
    const int32_t* m = manifest + (size_t)k * SDC_MARK_MANIFEST;
    int w = 0;
    if (m[SDC_MARK_M_LAYOUT] != layout) w = 1;
    else if (f.mark_engine_id == 0 || m[SDC_MARK_M_ENGINE] != f.mark_engine_id) w = 2;
    else if (m[SDC_MARK_M_ENV] != e) w = 3;
    else if (m[SDC_MARK_M_STEPS] != max_steps || m[SDC_MARK_M_HIST_CAP] != f.hist_cap) w = 4;
    else if (envs && row_of[(size_t)e] >= 0) w = 5;
    else if (!mir.mark_alive(e, m[SDC_MARK_M_SERIAL])) w = 6;
    else if (mir.steps_since(e, m[SDC_MARK_M_T_REL]) < 0) w = 7;
    else if (mir.steps_since(e, m[SDC_MARK_M_T_REL]) > max_steps) {
      w = 8;
      overrun.push_back(e);
    }
    if (envs) row_of[(size_t)e] = k;
    if (w && bad_k < 0) { bad_k = k; bad_why = w; }
  }
  if (bad_k < 0) return std::nullopt;
  const int e = envs ? envs[bad_k] : bad_k;
  const int32_t* m = manifest + (size_t)bad_k * SDC_MARK_MANIFEST;
  const int taken = mir.steps_since(e, m[SDC_MARK_M_T_REL]);
  switch (bad_why) {
    case 1: why = "state layout " + std::to_string(m[SDC_MARK_M_LAYOUT]) + ", this library's is " + std::to_string(layout); break;
    case 2: why = "the mark was taken from another engine (a mark goes back into the engine and the env it came from)"; break;
    case 3: why = "the mark was taken from env " + std::to_string(m[SDC_MARK_M_ENV]); break;
    case 4: why = "max_steps / hist_cap differ from the first row's / this engine's (the rows of a call come from one sdc_mark_envs call)"; break;
    case 5: why = "the env appears twice"; break;
    case 6: why = "the mark is dead (a later mark of the env, a reset, sdc_set_state, a clone or restore into the env, or an earlier "
                  "rewind refused beyond its max_steps)"; break;
    case 7: why = "the env is at episode step " + std::to_string(mir.t_rel(e)) + ", before the mark's " + std::to_string(m[SDC_MARK_M_T_REL]);
            break;
    default: why = std::to_string(taken) + " steps taken since the mark, more than its max_steps = " + std::to_string(max_steps) +
                   " (the mark is dead for good: slots beyond its reach have been overwritten)";
  }
  return "sdc_rewind_envs: row " + std::to_string(bad_k) + " (env " + std::to_string(e) + "): " + why;
}

// ---- the plan calls ---------------------------------------------------------------------------------------------------------------------
// (w: the caller's "who: ")
constexpr int SDC_FORECAST_N_CHANNELS = (int)(sizeof(sdc_plan_forecast::mode) / sizeof(int32_t));      // W, C, T, WB

// f: the forecast as it is stored, every field 0 for fc == NULL
static inline SdcMsg sdc_set_plan_forecast_refused(const SdcCallFacts& facts, const sdc_plan_forecast* fc, sdc_plan_forecast& f) {
  static const std::string w = "sdc_set_plan_forecast: ";
  if (!facts.handle) return w + "null handle";
  std::memset(&f, 0, sizeof(f));
  if (fc) {
    for (int c = 0; c < SDC_FORECAST_N_CHANNELS; c++) {
      if (fc->mode[c] < SDC_FORECAST_PERFECT || fc->mode[c] > SDC_FORECAST_VALUES)
        return w + "mode[" + std::to_string(c) + "] = " + std::to_string(fc->mode[c]) + " outside [0, 3]";
      f.mode[c] = fc->mode[c];
    }
    if (fc->values_entries < 0) return w + "values_entries = " + std::to_string(fc->values_entries) + " is negative";
    f.values_entries = fc->values_entries;
    f.values = fc->values;
  }
  return std::nullopt;
}

// a VALUES channel of the handle's forecast without n_entries entries to read
static inline SdcMsg sdc_forecast_values_refused(const std::string& w, const SdcCallFacts& facts, const int n_entries) {
  const sdc_plan_forecast& f = facts.forecast;
  for (int c = 0; c < SDC_FORECAST_N_CHANNELS; c++) {
    if (f.mode[c] != SDC_FORECAST_VALUES) continue;
    if (!f.values) return w + "forecast channel " + std::to_string(c) + " is SDC_FORECAST_VALUES and values is null";
    if (f.values_entries < n_entries)
      return w + "the forecast's values hold " + std::to_string(f.values_entries) + " entries, " + std::to_string(n_entries) +
             " are needed (n_steps + 2 at a plan call)";
  }
  return std::nullopt;
}
// what a plan call of n_steps refuses while a forecast is set (any channel not PERFECT)
static inline SdcMsg sdc_forecast_refused(const std::string& w, const SdcCallFacts& f, const int n_steps) {
  bool any = false;
  for (int c = 0; c < SDC_FORECAST_N_CHANNELS; c++) any = any || f.forecast.mode[c] != SDC_FORECAST_PERFECT;
  if (!any) return std::nullopt;
  if (!f.has_feat) return w + "this engine has no feature rows (episodes too long for them): the forecast lives in the feature rows";
  for (int e = 0; e < f.n_envs && f.mirror->n_feat() != f.n_envs; e++)      // (the count: no walk while every env's rows are valid)
    if (!f.mirror->feat(e))
      return w + "env " + std::to_string(e) +
             "'s feature rows are not valid (a host write to its state since its reset): the forecast lives in the feature rows";
  return sdc_forecast_values_refused(w, f, n_steps + 2);
}

static inline SdcMsg sdc_forecast_traces_refused(const SdcCallFacts& f, const int n_entries, const int truth, const double* out) {
  static const std::string w = "sdc_forecast_traces: ";
  if (!f.handle) return w + "null handle";
  if (n_entries < 1 || n_entries > SDC_MARK_MAX_STEPS + 2)
    return w + "n_entries = " + std::to_string(n_entries) + " outside [1, " + std::to_string(SDC_MARK_MAX_STEPS + 2) + "]";
  if (!out) return w + "null out";
  if ((sdc_addr_bits(out) & 7u) != 0) return w + "out not 8-byte aligned";
  if (!f.started) return w + "sdc_reset must be called first";
  if (n_entries > f.left + 2)
    return w + "n_entries = " + std::to_string(n_entries) + " reaches past the end of an episode (" + std::to_string(f.left) +
           " steps left: at most that + 2 entries)";
  if (!truth) return sdc_forecast_values_refused(w, f, n_entries);
  return std::nullopt;
}

// What every plan call refuses about its objective; obj: the objective with the defaults filled in
static inline SdcMsg sdc_plan_objective_refused(const std::string& w, const sdc_plan_objective* objective, sdc_plan_objective& obj) {
  std::memset(&obj, 0, sizeof(obj));
  obj.reward_weight[0] = obj.reward_weight[1] = obj.reward_weight[2] = 1.0;
  obj.gamma = 1.0;
  if (objective) obj = *objective;
  if (!(obj.gamma > 0.0 && obj.gamma <= 1.0)) return w + "gamma = " + std::to_string(obj.gamma) + " outside (0, 1]";
  if (obj.n_cols < 0 || obj.n_cols > SDC_PLAN_MAX_COLS)
    return w + "n_cols = " + std::to_string(obj.n_cols) + " outside [0, " + std::to_string(SDC_PLAN_MAX_COLS) + "]";
  for (int j = 0; j < obj.n_cols; j++)
    if (obj.col[j] < 0 || obj.col[j] >= SDC_INFO_DIM)
      return w + "info column " + std::to_string(obj.col[j]) + " (entry " + std::to_string(j) + ") outside [0, " +
             std::to_string(SDC_INFO_DIM) + ")";
  return std::nullopt;
}

// What every plan call refuses about the horizon, the engine and the objective, in sdc_plan's order (`arrays`: the caller's own null
// check, reported at its place in that order)
static inline SdcMsg sdc_plan_common_refused(const std::string& w, const SdcCallFacts& f, const int n_steps, const bool arrays, const float* obs,
                                      const float* share_obs, const sdc_plan_objective* objective, sdc_plan_objective& obj) {
  if (n_steps < 1 || n_steps > SDC_MARK_MAX_STEPS)
    return w + "n_steps = " + std::to_string(n_steps) + " outside [1, " + std::to_string(SDC_MARK_MAX_STEPS) + "]";
  if (!arrays || !obs || !share_obs) return w + "null array";
  if ((sdc_addr_bits(obs, share_obs) & 3u) != 0) return w + "obs / share_obs rows not dword-aligned";
  if (!f.started) return w + "sdc_reset must be called first";
  if (f.debug_flags & SDC_DEBUG_VERIFY) return w + "verify mode checks single steps (sdc_rollout refuses it as well)";
  if (f.auto_reset && n_steps >= f.left)
    return w + "n_steps = " + std::to_string(n_steps) + " would finish an episode (" + std::to_string(f.left) +
           " steps left): the auto-reset kills the mark";
  if (n_steps > f.left)
    return w + "n_steps = " + std::to_string(n_steps) + " would run past the end of an episode (" + std::to_string(f.left) + " steps left)";
  if (SdcMsg m = sdc_plan_objective_refused(w, objective, obj)) return m;
  return sdc_forecast_refused(w, f, n_steps);
}

static inline SdcMsg sdc_plan_refused(const SdcCallFacts& f, const int n_cand, const int n_steps, const int32_t* actions,
                               const sdc_plan_objective* objective, const double* score, const int32_t* best, const int32_t* best_action,
                               const float* obs, const float* share_obs, sdc_plan_objective& obj) {
  if (!f.handle) return "sdc_plan: null handle";
  if (n_cand < 1) return "sdc_plan: n_cand = " + std::to_string(n_cand) + " must be positive";
  return sdc_plan_common_refused("sdc_plan: ", f, n_steps, actions && score && best && best_action, obs, share_obs, objective, obj);
}

// t: the terms as they are stored, every field 0 for terms == NULL or both counts 0
static inline SdcMsg sdc_set_plan_terms_refused(const SdcCallFacts& f, const sdc_plan_terms* terms, sdc_plan_terms& t) {
  static const std::string w = "sdc_set_plan_terms: ";
  if (!f.handle) return w + "null handle";
  std::memset(&t, 0, sizeof(t));
  if (!terms || (terms->n_limits == 0 && terms->n_terminal == 0)) return std::nullopt;
  if (terms->n_limits < 0 || terms->n_limits > SDC_PLAN_MAX_LIMITS)
    return w + "n_limits = " + std::to_string(terms->n_limits) + " outside [0, " + std::to_string(SDC_PLAN_MAX_LIMITS) + "]";
  if (terms->n_terminal < 0 || terms->n_terminal > SDC_PLAN_MAX_TERMINAL)
    return w + "n_terminal = " + std::to_string(terms->n_terminal) + " outside [0, " + std::to_string(SDC_PLAN_MAX_TERMINAL) + "]";
  const auto entry = [](const char* field, const int j) { return std::string(field) + "[" + std::to_string(j) + "] = "; };
  t.n_limits = terms->n_limits;
  t.n_terminal = terms->n_terminal;
  for (int j = 0; j < t.n_limits; j++) {
    const int col = terms->limit_col[j], side = terms->limit_side[j];
    const double bound = terms->limit_bound[j], weight = terms->limit_weight[j];
    if (col < 0 || col >= SDC_INFO_DIM)
      return w + entry("limit_col", j) + std::to_string(col) + " outside [0, " + std::to_string(SDC_INFO_DIM) + ")";
    if (side != 1 && side != -1) return w + entry("limit_side", j) + std::to_string(side) + " is neither +1 (upper) nor -1 (lower)";
    if (!std::isfinite(bound)) return w + entry("limit_bound", j) + std::to_string(bound) + " is not finite";
    if (!std::isfinite(weight)) return w + entry("limit_weight", j) + std::to_string(weight) + " is not finite";
    if (weight < 0.0) return w + entry("limit_weight", j) + std::to_string(weight) + " is negative";
    t.limit_col[j] = col;
    t.limit_side[j] = side;
    t.limit_bound[j] = bound;
    t.limit_weight[j] = weight;
  }
  for (int j = 0; j < t.n_terminal; j++) {
    const int col = terms->terminal_col[j];
    const double weight = terms->terminal_weight[j];
    if (col < 0 || col >= SDC_INFO_DIM)
      return w + entry("terminal_col", j) + std::to_string(col) + " outside [0, " + std::to_string(SDC_INFO_DIM) + ")";
    if (!std::isfinite(weight)) return w + entry("terminal_weight", j) + std::to_string(weight) + " is not finite";
    t.terminal_col[j] = col;
    t.terminal_weight[j] = weight;
  }
  return std::nullopt;
}

// ---- the critic ---------------------------------------------------------------------------------------------------------------------------
// (what is refused about the parameters themselves: sdc_critic_pack.hpp sdc_critic_params_error, which reads every float of the struct)
static inline SdcMsg sdc_set_critic_refused(const SdcCallFacts& f, const sdc_critic_params* p) {
  static const std::string w = "sdc_set_critic: ";
  if (!f.handle || !p) return w + "null handle or params";
  if (const char* why = sdc_critic_params_error(p)) return w + why;
  return std::nullopt;
}

static inline SdcMsg sdc_critic_values_refused(const SdcCallFacts& f, const float* share_obs, const long long n_rows, const float* values) {
  static const std::string w = "sdc_critic_values: ";
  if (!f.handle) return w + "null handle";
  if (!f.critic_set) return w + "sdc_set_critic first";
  if (n_rows < 1) return w + "n_rows = " + std::to_string(n_rows) + " must be positive";
  if (!share_obs || !values) return w + "null array";
  if ((sdc_addr_bits(share_obs, values) & 3u) != 0) return w + "share_obs / values not dword-aligned";
  return std::nullopt;
}
static inline SdcMsg sdc_set_plan_critic_refused(const SdcCallFacts& f, const double weight) {
  static const std::string w = "sdc_set_plan_critic: ";
  if (!f.handle) return w + "null handle";
  if (!std::isfinite(weight)) return w + "weight = " + std::to_string(weight) + " is not finite";
  if (weight != 0.0 && !f.critic_set) return w + "weight = " + std::to_string(weight) + " while no critic is set (sdc_set_critic first)";
  return std::nullopt;
}

// ---- the on-policy batch ------------------------------------------------------------------------------------------------------------------
// (pure functions of their arrays: nothing about the engine's episode is asked; their texts are held by tests/test_onpolicy_abi.py)
static inline SdcMsg sdc_gae_refused(const SdcCallFacts& f, const int n_steps, const float* rew, const int reward_agent, const uint8_t* done,
                                     const float* values, const double gamma, const double gae_lambda, const int use_gae, const float* returns,
                                     const float* advantages, const float* masks, const float* value_preds, const double* moments) {
  static const std::string w = "sdc_gae: ";
  if (!f.handle) return w + "null handle";
  if (n_steps < 1) return w + "n_steps = " + std::to_string(n_steps) + " must be positive";
  if (!rew || !done || !values || !returns || !advantages || !masks)
    return w + "null array (rew, done, values, returns, advantages and masks are required)";
  if ((sdc_addr_bits(rew, values, returns, advantages, masks, value_preds) & 3u) != 0)
    return w + "rew / values / returns / advantages / masks / value_preds not dword-aligned";
  if ((sdc_addr_bits(moments) & 15u) != 0) return w + "moments not 16-byte aligned";
  if (reward_agent < 0 || reward_agent > 2) return w + "reward_agent = " + std::to_string(reward_agent) + " outside [0, 2]";
  if (use_gae != 0 && use_gae != 1) return w + "use_gae = " + std::to_string(use_gae) + " outside {0, 1}";
  if (!(gamma >= 0.0 && gamma <= 1.0)) return w + "gamma = " + std::to_string(gamma) + " outside [0, 1]";
  if (!(gae_lambda >= 0.0 && gae_lambda <= 1.0)) return w + "gae_lambda = " + std::to_string(gae_lambda) + " outside [0, 1]";
  if (value_preds && !f.critic_set) return w + "value_preds asked for while no critic is set (sdc_set_critic first: its scale and shift)";
  return std::nullopt;
}
static inline SdcMsg sdc_action_log_probs_refused(const SdcCallFacts& f, const int n_steps, const int32_t* actions, const float* logits,
                                                  const float* log_probs, const float* entropy) {
  static const std::string w = "sdc_action_log_probs: ";
  if (!f.handle) return w + "null handle";
  if (n_steps < 1) return w + "n_steps = " + std::to_string(n_steps) + " must be positive";
  if (!actions || !logits || !log_probs) return w + "null array (actions, logits and log_probs are required)";
  if ((sdc_addr_bits(actions, logits, log_probs, entropy) & 3u) != 0) return w + "actions / logits / log_probs / entropy not dword-aligned";
  return std::nullopt;
}

// ---- the actors on stored rows, and the PPO terms --------------------------------------------------------------------------------------------
// (pure functions of their arrays, as the on-policy batch's; their texts are held by tests/test_actor_eval_abi.py)
static inline SdcMsg sdc_actor_evaluate_refused(const SdcCallFacts& f, const int agent_slot, const float* obs, const long long row_stride,
                                                const long long n_rows, const float* logits, const long long logits_stride) {
  static const std::string w = "sdc_actor_evaluate: ";
  if (!f.handle) return w + "null handle";
  if (agent_slot < 0 || agent_slot > 2) return w + "agent_slot = " + std::to_string(agent_slot) + " outside [0, 2]";
  if (!f.actor_set[agent_slot]) return w + "no actor is set for agent_slot " + std::to_string(agent_slot) + " (sdc_set_actor first)";
  if (n_rows < 1) return w + "n_rows = " + std::to_string(n_rows) + " must be positive";
  if (!obs || !logits) return w + "null array (obs and logits are required)";
  if ((sdc_addr_bits(obs, logits) & 3u) != 0) return w + "obs / logits not dword-aligned";
  if (row_stride < 26) return w + "row_stride = " + std::to_string(row_stride) + " below a row's 26 floats";
  if (logits_stride < 3) return w + "logits_stride = " + std::to_string(logits_stride) + " below a row's 3 floats";
  return std::nullopt;
}
static inline SdcMsg sdc_ppo_terms_refused(const SdcCallFacts& f, const int n_steps, const int agent, const float* new_log_probs,
                                           const float* old_log_probs, const float* entropy, const float* advantages, const float* factor,
                                           const double clip_param, const float* ratio, const float* surr, const float* factor_out,
                                           const double* stats) {
  static const std::string w = "sdc_ppo_terms: ";
  if (!f.handle) return w + "null handle";
  if (n_steps < 1) return w + "n_steps = " + std::to_string(n_steps) + " must be positive";
  if (agent < 0 || agent > 2) return w + "agent = " + std::to_string(agent) + " outside [0, 2]";
  if (!new_log_probs || !old_log_probs || !advantages || !ratio)
    return w + "null array (new_log_probs, old_log_probs, advantages and ratio are required)";
  if ((sdc_addr_bits(new_log_probs, old_log_probs, entropy, advantages, factor, ratio, surr, factor_out) & 3u) != 0)
    return w + "new_log_probs / old_log_probs / entropy / advantages / factor / ratio / surr / factor_out not dword-aligned";
  if ((sdc_addr_bits(stats) & 7u) != 0) return w + "stats not 8-byte aligned";
  if (!(clip_param >= 0.0 && clip_param < 1.0)) return w + "clip_param = " + std::to_string(clip_param) + " outside [0, 1)";
  return std::nullopt;
}

// ---- the actors' gradient --------------------------------------------------------------------------------------------------------------------
// (pure functions of their arrays, as the calls above; their texts are held by tests/test_actor_grad_abi.py)
static inline SdcMsg sdc_ppo_dlogp_refused(const SdcCallFacts& f, const int n_steps, const int agent, const float* new_log_probs,
                                           const float* old_log_probs, const float* advantages, const float* factor, const double clip_param,
                                           const double scale, const float* dlogp) {
  static const std::string w = "sdc_ppo_dlogp: ";
  if (!f.handle) return w + "null handle";
  if (n_steps < 1) return w + "n_steps = " + std::to_string(n_steps) + " must be positive";
  if (agent < 0 || agent > 2) return w + "agent = " + std::to_string(agent) + " outside [0, 2]";
  if (!new_log_probs || !old_log_probs || !advantages || !dlogp)
    return w + "null array (new_log_probs, old_log_probs, advantages and dlogp are required)";
  if ((sdc_addr_bits(new_log_probs, old_log_probs, advantages, factor, dlogp) & 3u) != 0)
    return w + "new_log_probs / old_log_probs / advantages / factor / dlogp not dword-aligned";
  if (!(clip_param >= 0.0 && clip_param < 1.0)) return w + "clip_param = " + std::to_string(clip_param) + " outside [0, 1)";
  if (!std::isfinite(scale)) return w + "scale = " + std::to_string(scale) + " is not finite";
  return std::nullopt;
}
static inline SdcMsg sdc_actor_backward_refused(const SdcCallFacts& f, const int agent_slot, const float* obs, const long long row_stride,
                                                const long long n_rows, const int32_t* actions, const long long action_stride,
                                                const float* dlogp, const double dent, const float* grads, const double* grad_sq) {
  static const std::string w = "sdc_actor_backward: ";
  if (!f.handle) return w + "null handle";
  if (agent_slot < 0 || agent_slot > 2) return w + "agent_slot = " + std::to_string(agent_slot) + " outside [0, 2]";
  if (!f.actor_set[agent_slot]) return w + "no actor is set for agent_slot " + std::to_string(agent_slot) + " (sdc_set_actor first)";
  if (n_rows < 1) return w + "n_rows = " + std::to_string(n_rows) + " must be positive";
  if (!obs || !actions || !dlogp || !grads) return w + "null array (obs, actions, dlogp and grads are required)";
  if ((sdc_addr_bits(obs, actions, dlogp, grads) & 3u) != 0) return w + "obs / actions / dlogp / grads not dword-aligned";
  if ((sdc_addr_bits(grad_sq) & 7u) != 0) return w + "grad_sq not 8-byte aligned";
  if (row_stride < 26) return w + "row_stride = " + std::to_string(row_stride) + " below a row's 26 floats";
  if (action_stride < 1) return w + "action_stride = " + std::to_string(action_stride) + " must be positive";
  if (!std::isfinite(dent)) return w + "dent = " + std::to_string(dent) + " is not finite";
  return std::nullopt;
}

// ---- the critic's gradient -------------------------------------------------------------------------------------------------------------------
// (pure functions of their arrays, as the calls above; their texts are held by tests/test_critic_grad_abi.py)
static inline SdcMsg sdc_critic_evaluate_refused(const SdcCallFacts& f, const float* share_obs, const long long n_rows, const float* raw_values) {
  static const std::string w = "sdc_critic_evaluate: ";
  if (!f.handle) return w + "null handle";
  if (!f.critic_set) return w + "sdc_set_critic first";
  if (n_rows < 1) return w + "n_rows = " + std::to_string(n_rows) + " must be positive";
  if (!share_obs || !raw_values) return w + "null array";
  if ((sdc_addr_bits(share_obs, raw_values) & 3u) != 0) return w + "share_obs / raw_values not dword-aligned";
  return std::nullopt;
}
static inline SdcMsg sdc_value_loss_refused(const SdcCallFacts& f, const long long n, const float* raw_values, const float* value_preds,
                                            const float* returns, const double target_scale, const double target_shift, const double clip_param,
                                            const double huber_delta, const int flags, const double coef, const float* loss, const float* dvalue,
                                            const double* stats) {
  static const std::string w = "sdc_value_loss: ";
  if (!f.handle) return w + "null handle";
  if (n < 1) return w + "n = " + std::to_string(n) + " must be positive";
  if (!raw_values || !value_preds || !returns || !dvalue) return w + "null array (raw_values, value_preds, returns and dvalue are required)";
  if ((sdc_addr_bits(raw_values, value_preds, returns, loss, dvalue) & 3u) != 0)
    return w + "raw_values / value_preds / returns / loss / dvalue not dword-aligned";
  if ((sdc_addr_bits(stats) & 7u) != 0) return w + "stats not 8-byte aligned";
  if (!(std::isfinite(target_scale) && target_scale > 0.0)) return w + "target_scale = " + std::to_string(target_scale) + " must be finite and positive";
  if (!std::isfinite(target_shift)) return w + "target_shift = " + std::to_string(target_shift) + " is not finite";
  if (!(std::isfinite(clip_param) && clip_param >= 0.0)) return w + "clip_param = " + std::to_string(clip_param) + " must be finite and not negative";
  if (flags < 0 || (flags >> 2) != 0) return w + "flags = " + std::to_string(flags) + ": unknown bits (bit 0: Huber loss, bit 1: clipped value loss)";
  if ((flags & 1) != 0 && !(std::isfinite(huber_delta) && huber_delta > 0.0))
    return w + "huber_delta = " + std::to_string(huber_delta) + " must be finite and positive";
  if (!std::isfinite(coef)) return w + "coef = " + std::to_string(coef) + " is not finite";
  return std::nullopt;
}
static inline SdcMsg sdc_critic_backward_refused(const SdcCallFacts& f, const float* share_obs, const long long n_rows, const float* dvalue,
                                                 const float* grads, const double* grad_sq) {
  static const std::string w = "sdc_critic_backward: ";
  if (!f.handle) return w + "null handle";
  if (!f.critic_set) return w + "sdc_set_critic first";
  if (n_rows < 1) return w + "n_rows = " + std::to_string(n_rows) + " must be positive";
  if (!share_obs || !dvalue || !grads) return w + "null array (share_obs, dvalue and grads are required)";
  if ((sdc_addr_bits(share_obs, dvalue, grads) & 3u) != 0) return w + "share_obs / dvalue / grads not dword-aligned";
  if ((sdc_addr_bits(grad_sq) & 7u) != 0) return w + "grad_sq not 8-byte aligned";
  return std::nullopt;
}

// ---- the optimiser step ------------------------------------------------------------------------------------------------------------------------
// (what is refused about an sdc_adam and an sdc_optim_state: sdc_optim.hpp; the texts are held by tests/test_optim_abi.py.  `who`: the
// entry point; agent_slot < 0 where `who` is one of the critic's: its rule about the network is "sdc_set_critic first")
static inline SdcMsg sdc_optim_network_refused(const std::string& w, const SdcCallFacts& f, const bool actor, const int agent_slot) {
  if (!f.handle) return w + "null handle";
  if (actor) {
    if (agent_slot < 0 || agent_slot > 2) return w + "agent_slot = " + std::to_string(agent_slot) + " outside [0, 2]";
    if (!f.actor_set[agent_slot]) return w + "no actor is set for agent_slot " + std::to_string(agent_slot) + " (sdc_set_actor first)";
  } else if (!f.critic_set) {
    return w + "sdc_set_critic first";
  }
  return std::nullopt;
}
static inline SdcMsg sdc_adam_step_refused(const char* who, const SdcCallFacts& f, const bool actor, const int agent_slot, const float* grads,
                                           const sdc_adam* adam, const double* grad_norm) {
  const std::string w = std::string(who) + ": ";
  if (SdcMsg m = sdc_optim_network_refused(w, f, actor, agent_slot)) return m;
  if (!grads) return w + "null grads";
  if ((sdc_addr_bits(grads) & 3u) != 0) return w + "grads not dword-aligned";
  if ((sdc_addr_bits(grad_norm) & 7u) != 0) return w + "grad_norm not 8-byte aligned";
  if (const char* why = sdc_adam_error(adam)) return w + why;
  return std::nullopt;
}
// sdc_get_actor / sdc_get_critic / sdc_get_*_optim: `out_ok`: every output pointer is there
static inline SdcMsg sdc_optim_get_refused(const char* who, const SdcCallFacts& f, const bool actor, const int agent_slot, const bool out_ok) {
  const std::string w = std::string(who) + ": ";
  if (SdcMsg m = sdc_optim_network_refused(w, f, actor, agent_slot)) return m;
  if (!out_ok) return w + "null output";
  return std::nullopt;
}
static inline SdcMsg sdc_set_optim_refused(const char* who, const SdcCallFacts& f, const bool actor, const int agent_slot, const float* m,
                                           const float* v, const sdc_optim_state* st) {
  const std::string w = std::string(who) + ": ";
  if (SdcMsg msg = sdc_optim_network_refused(w, f, actor, agent_slot)) return msg;
  if (const char* why = sdc_optim_state_error(m, v, st, actor ? SDC_ACTOR_N_PARAMS : SDC_CRITIC_N_PARAMS)) return w + why;
  return std::nullopt;
}
static inline SdcMsg sdc_set_critic_norm_refused(const SdcCallFacts& f, const double scale, const double shift) {
  static const std::string w = "sdc_set_critic_norm: ";
  if (SdcMsg m = sdc_optim_network_refused(w, f, false, -1)) return m;
  if (!std::isfinite((float)scale) || !std::isfinite((float)shift)) return w + "an entry that is not finite";
  if (!((float)scale > 0.0f)) return w + "scale must be positive";
  return std::nullopt;
}

// ---- train on the device: permutation, gather, ValueNorm ------------------------------------------------------------------------------------
// (what is refused about an sdc_value_norm and a gather segment: sdc_minibatch.hpp; the texts are held by tests/test_train_abi.py.
// `installed`: the handle holds a ValueNorm)
static inline SdcMsg sdc_permutation_refused(const SdcCallFacts& f, const long long n, const int32_t* perm) {
  static const std::string w = "sdc_permutation: ";
  if (!f.handle) return w + "null handle";
  if (n < 1 || n > SDC_PERM_MAX_N) return w + "n = " + std::to_string(n) + " outside [1, 2147483647]";
  if (!perm) return w + "null perm";
  if ((sdc_addr_bits(perm) & 3u) != 0) return w + "perm not dword-aligned";
  return std::nullopt;
}
static inline SdcMsg sdc_gather_rows_refused(const SdcCallFacts& f, const int32_t* idx, const long long n_rows, const long long n_src_rows,
                                             const sdc_gather_segment* segs, const int n_segs, const int32_t* bad) {
  static const std::string w = "sdc_gather_rows: ";
  if (!f.handle) return w + "null handle";
  if (n_rows < 1) return w + "n_rows = " + std::to_string(n_rows) + " must be positive";
  if (n_src_rows < 1 || n_src_rows > SDC_PERM_MAX_N) return w + "n_src_rows = " + std::to_string(n_src_rows) + " outside [1, 2147483647]";
  if (!idx || !segs) return w + "null idx or segs";
  if ((sdc_addr_bits(idx, bad) & 3u) != 0) return w + "idx / bad not dword-aligned";
  if (n_segs < 1 || n_segs > SDC_GATHER_MAX_SEGMENTS)
    return w + "n_segs = " + std::to_string(n_segs) + " outside [1, " + std::to_string(SDC_GATHER_MAX_SEGMENTS) + "]";
  static const char* const why[4] = {"a null src or dst", "src / dst not dword-aligned", "n_dwords must be positive",
                                     "a stride below n_dwords"};
  for (int g = 0; g < n_segs; g++) {
    const int e = sdc_gather_segment_error(segs[g]);
    if (e >= 0) return w + "segment " + std::to_string(g) + ": " + why[e];
  }
  return std::nullopt;
}
static inline SdcMsg sdc_set_value_norm_refused(const SdcCallFacts& f, const sdc_value_norm* st) {
  static const std::string w = "sdc_set_value_norm: ";
  if (SdcMsg m = sdc_optim_network_refused(w, f, false, -1)) return m;
  if (st)
    if (const char* e = sdc_value_norm_error(st)) return w + e;
  return std::nullopt;
}
static inline SdcMsg sdc_get_value_norm_refused(const SdcCallFacts& f, const bool installed, const sdc_value_norm* out) {
  static const std::string w = "sdc_get_value_norm: ";
  if (SdcMsg m = sdc_optim_network_refused(w, f, false, -1)) return m;
  if (!installed) return w + "no ValueNorm is installed (sdc_set_value_norm first)";
  if (!out) return w + "null output";
  return std::nullopt;
}
static inline SdcMsg sdc_value_norm_update_refused(const SdcCallFacts& f, const bool installed, const float* returns, const long long n,
                                                   const double beta) {
  static const std::string w = "sdc_value_norm_update: ";
  if (SdcMsg m = sdc_optim_network_refused(w, f, false, -1)) return m;
  if (!installed) return w + "no ValueNorm is installed (sdc_set_value_norm first)";
  if (n < 1) return w + "n = " + std::to_string(n) + " must be positive";
  if (!returns) return w + "null returns";
  if ((sdc_addr_bits(returns) & 3u) != 0) return w + "returns not dword-aligned";
  if (!(beta >= 0.0 && beta < 1.0)) return w + "beta = " + std::to_string(beta) + " outside [0, 1)";
  return std::nullopt;
}
// (sdc_value_loss' rule under this call's name, with the block's scale and shift standing in as 1 and 0)
static inline SdcMsg sdc_value_loss_normed_refused(const SdcCallFacts& f, const bool installed, const long long n, const float* raw_values,
                                                   const float* value_preds, const float* returns, const double clip_param,
                                                   const double huber_delta, const int flags, const double coef, const float* loss,
                                                   const float* dvalue, const double* stats) {
  static const std::string w = "sdc_value_loss_normed: ";
  if (SdcMsg m = sdc_value_loss_refused(f, n, raw_values, value_preds, returns, 1.0, 0.0, clip_param, huber_delta, flags, coef, loss, dvalue, stats))
    return w + m->substr(std::strlen("sdc_value_loss: "));
  if (!installed) return w + "no ValueNorm is installed (sdc_set_value_norm first)";
  return std::nullopt;
}

// ---- the cross-entropy planners -------------------------------------------------------------------------------------------------------------
// The parameter ranges sdc_plan_cem and sdc_plan_cem_groups refuse alike.  The callers run them in their own order.
static inline SdcMsg sdc_cem_iters_refused(const std::string& w, const int n_iters, const int iter0) {
  if (n_iters < 1) return w + "n_iters = " + std::to_string(n_iters) + " must be positive";
  if (iter0 < 0 || (long long)iter0 + n_iters > 65536)
    return w + "iter0 = " + std::to_string(iter0) + " with n_iters = " + std::to_string(n_iters) + " outside [0, 65536]";
  return std::nullopt;
}
// (the population the elites are taken from: its name and size)
static inline SdcMsg sdc_cem_elite_refused(const std::string& w, const int n_elite, const char* pop, const int size) {
  if (n_elite < 1 || n_elite > size)
    return w + "n_elite = " + std::to_string(n_elite) + " outside [1, " + pop + " = " + std::to_string(size) + "]";
  return std::nullopt;
}
static inline SdcMsg sdc_cem_refit_refused(const std::string& w, const int32_t* fixed_action, const double alpha, const double p_min) {
  for (int a = 0; a < 3; a++)
    if (fixed_action[a] < -1 || fixed_action[a] > 2)
      return w + "fixed_action[" + std::to_string(a) + "] = " + std::to_string(fixed_action[a]) + " outside [-1, 2]";
  if (!(alpha >= 0.0 && alpha < 1.0)) return w + "alpha = " + std::to_string(alpha) + " outside [0, 1)";
  if (!(p_min >= 0.0 && p_min <= 1.0 / 3.0)) return w + "p_min = " + std::to_string(p_min) + " outside [0, 1/3]";
  return std::nullopt;
}
// What sdc_plan_cem and sdc_rollout_cem_stats refuse alike about the per-env planner's parameters, in the former's order
static inline SdcMsg sdc_cem_params_refused(const std::string& w, const sdc_cem_params& c) {
  if (SdcMsg m = sdc_cem_iters_refused(w, c.n_iters, c.iter0)) return m;
  if (c.n_cand < 2 || c.n_cand > SDC_CEM_MAX_CAND)
    return w + "n_cand = " + std::to_string(c.n_cand) + " outside [2, " + std::to_string(SDC_CEM_MAX_CAND) + "]";
  if (SdcMsg m = sdc_cem_elite_refused(w, c.n_elite, "n_cand", c.n_cand)) return m;
  return sdc_cem_refit_refused(w, c.fixed_action, c.alpha, c.p_min);
}
// What sdc_plan_cem_groups and sdc_rollout_cem_groups_stats refuse alike about the groups of a batch of N envs, in the former's order
static inline SdcMsg sdc_cem_groups_refused(const std::string& w, const int N, const sdc_cem_group_params& c) {
  if (c.group_size < 2 || c.group_size > SDC_CEM_MAX_GROUP)
    return w + "group_size = " + std::to_string(c.group_size) + " outside [2, " + std::to_string(SDC_CEM_MAX_GROUP) + "]";
  if (N % c.group_size != 0) return w + "n_envs = " + std::to_string(N) + " is not a multiple of group_size = " + std::to_string(c.group_size);
  if (SdcMsg m = sdc_cem_elite_refused(w, c.n_elite, "group_size", c.group_size)) return m;
  if (c.group_base < 0) return w + "group_base = " + std::to_string(c.group_base) + " is negative";
  return std::nullopt;
}
// the three of them in the group calls' order
static inline SdcMsg sdc_cem_group_params_refused(const std::string& w, const int N, const sdc_cem_group_params& c) {
  if (SdcMsg m = sdc_cem_iters_refused(w, c.n_iters, c.iter0)) return m;
  if (SdcMsg m = sdc_cem_groups_refused(w, N, c)) return m;
  return sdc_cem_refit_refused(w, c.fixed_action, c.alpha, c.p_min);
}
// ... and, from what the host's mirror knows of a group's replicas in O(N): the episode step, the config, the trace set, the
// feature-row flag
static inline SdcMsg sdc_groups_out_of_step_refused(const std::string& w, const SdcCallFacts& f, const int R) {
  const SdcHostMirror& mir = *f.mirror;
  for (int e = 0; e < f.n_envs; e++) {
    const int l = e - e % R;      // the group's first env
    if (e == l) continue;
    const char* what = mir.t_rel(e) != mir.t_rel(l)   ? "episode step"
                       : mir.cfg(e) != mir.cfg(l)     ? "data-centre config"
                       : mir.loc(e) != mir.loc(l)     ? "location"
                       : mir.feat(e) != mir.feat(l)   ? "feature-row flag"
                                                      : nullptr;
    if (what)
      return w + "group " + std::to_string(e / R) + " is out of step: env " + std::to_string(e) + " and its group's first env " +
             std::to_string(l) + " differ in " + what + " (the replicas of a group hold one state: sdc_clone_envs)";
  }
  return std::nullopt;
}

static inline SdcMsg sdc_plan_cem_refused(const SdcCallFacts& f, const int n_steps, const sdc_cem_params* cem, const sdc_plan_objective* objective,
                                   const double* probs, const int32_t* best_seq, const double* best_score, const int32_t* best_action,
                                   const int32_t* cand, const double* cand_score, const float* obs, const float* share_obs,
                                   sdc_plan_objective& obj) {
  static const std::string w = "sdc_plan_cem: ";
  if (!f.handle) return w + "null handle";
  if (!cem) return w + "null cem";
  if (SdcMsg m = sdc_cem_params_refused(w, *cem)) return m;
  return sdc_plan_common_refused(w, f, n_steps, probs && best_seq && best_score && best_action && cand && cand_score, obs, share_obs,
                                 objective, obj);
}

static inline SdcMsg sdc_plan_cem_groups_refused(const SdcCallFacts& f, const int n_steps, const sdc_cem_group_params* cem,
                                          const sdc_plan_objective* objective, const double* probs, const int32_t* best_seq,
                                          const double* best_score, const int32_t* best_action, const int32_t* step_actions,
                                          const int32_t* cand, const double* cand_score, const float* obs, const float* share_obs,
                                          sdc_plan_objective& obj) {
  static const std::string w = "sdc_plan_cem_groups: ";
  if (!f.handle) return w + "null handle";
  if (!cem) return w + "null cem";
  if (SdcMsg m = sdc_cem_group_params_refused(w, f.n_envs, *cem)) return m;
  if (SdcMsg m = sdc_plan_common_refused(w, f, n_steps, probs && best_seq && best_score && best_action && step_actions && cand && cand_score,
                                         obs, share_obs, objective, obj))
    return m;
  return sdc_groups_out_of_step_refused(w, f, cem->group_size);
}

// ---- episode statistics and planner evaluation ----------------------------------------------------------------------------------------------
// the caller's arrays of the statistics calls
struct SdcStatsArrays {
  double *stats, *returns;
  int32_t* counts;
  float *obs, *share_obs, *rew;
  uint8_t* done;
  float *info, *final_obs;
};

// What the four calls refuse about their arrays and the engine, in sdc_rollout_stats' order, up to verify mode
static inline SdcMsg sdc_stats_common_refused(const std::string& w, const SdcCallFacts& f, const int n_steps, const int accumulate,
                                       const SdcStatsArrays& a) {
  if (!f.handle) return w + "null handle";
  if (n_steps < 1) return w + "n_steps = " + std::to_string(n_steps) + " must be positive";
  if (!a.stats || !a.returns || !a.counts || !a.obs || !a.share_obs)
    return w + "null array (stats, returns, counts, obs and share_obs are required)";
  if ((sdc_addr_bits(a.stats, a.returns) & 15u) != 0) return w + "stats / returns not 16-byte aligned";
  if ((sdc_addr_bits(a.counts, a.obs, a.share_obs, a.rew, a.info, a.final_obs) & 3u) != 0)
    return w + "counts / obs / share_obs / rew / info / final_obs rows not dword-aligned";
  if (accumulate != 0 && accumulate != 1) return w + "accumulate = " + std::to_string(accumulate) + " outside {0, 1}";
  if (!f.started) return w + "sdc_reset must be called first";
  if (f.debug_flags & SDC_DEBUG_VERIFY) return w + "verify mode checks single steps (sdc_rollout refuses it as well)";
  return std::nullopt;
}
// ... and about the episode's end, `left` steps away (the mirror's steps_to_terminal, or what a sync will make of it)
static inline SdcMsg sdc_stats_past_end_refused(const std::string& w, const int n_steps, const int left) {
  if (n_steps > left)
    return w + "n_steps = " + std::to_string(n_steps) + " would run past the end of an episode (" + std::to_string(left) + " steps left)";
  return std::nullopt;
}

static inline SdcMsg sdc_rollout_stats_refused(const SdcCallFacts& f, const int n_steps, const int32_t* actions, const int accumulate,
                                        const SdcStatsArrays& a) {
  static const std::string w = "sdc_rollout_stats: ";
  if (SdcMsg m = sdc_stats_common_refused(w, f, n_steps, accumulate, a)) return m;
  if (!actions && !f.all_policies) return w + "actions may only be NULL when every agent slot has a policy";
  return sdc_stats_past_end_refused(w, n_steps, f.left);
}

// (f.step: step_facts without the call's arrays -- the rollouts go into the handle's block, all there and aligned --, share_obs, info
// and actions_out given.  What sdc_rollout_actor would refuse about the actors and the batch is asked here, before anything is enqueued)
static inline SdcMsg sdc_rollout_actor_stats_refused(const SdcCallFacts& f, const int n_steps, const int sample, const int accumulate,
                                              const SdcStatsArrays& a, const int32_t* policy_counts, const double* policy_sums) {
  static const std::string w = "sdc_rollout_actor_stats: ";
  if (SdcMsg m = sdc_stats_common_refused(w, f, n_steps, accumulate, a)) return m;
  if (sample != 0 && sample != 1) return w + "sample = " + std::to_string(sample) + " outside {0, 1}";
  if ((policy_counts == nullptr) != (policy_sums == nullptr)) return w + "policy_counts and policy_sums are given together or not at all";
  if ((sdc_addr_bits(policy_sums) & 15u) != 0) return w + "policy_sums not 16-byte aligned";
  if ((sdc_addr_bits(policy_counts) & 3u) != 0) return w + "policy_counts not dword-aligned";
  if (!sdc_actors_all_set(f)) return w + SDC_ACTORS_NOT_SET;
  if (!sdc_actors_one_activation(f)) return w + SDC_ACTORS_ACTIVATION;
  if (!f.latch_valid) return w + SDC_ACTORS_NO_OBS;
  if (sdc_actor_path(f.step).refused) return w + SDC_ACTORS_COMMON_CASE;
  return sdc_stats_past_end_refused(w, n_steps, f.left);
}

// What both planner evaluations refuse about the loop's own parameters (the leading fields of sdc_mpc_params and sdc_mpc_group_params)
static inline SdcMsg sdc_mpc_loop_refused(const std::string& w, const int H, const int warm_start, const int resume, const int resume_steps,
                                   const int32_t* idle_action) {
  if (H < 1 || H > SDC_MARK_MAX_STEPS) return w + "horizon = " + std::to_string(H) + " outside [1, " + std::to_string(SDC_MARK_MAX_STEPS) + "]";
  if (warm_start != 0 && warm_start != 1) return w + "warm_start = " + std::to_string(warm_start) + " outside {0, 1}";
  if (resume != 0 && resume != 1) return w + "resume = " + std::to_string(resume) + " outside {0, 1}";
  if (resume && (resume_steps < 1 || resume_steps > H))
    return w + "resume_steps = " + std::to_string(resume_steps) + " outside [1, horizon = " + std::to_string(H) + "]";
  for (int k = 0; k < 3; k++)
    if (idle_action[k] < 0 || idle_action[k] > 2)
      return w + "idle_action[" + std::to_string(k) + "] = " + std::to_string(idle_action[k]) + " outside [0, 2]";
  return std::nullopt;
}

// A caller's array under the name the messages give it, and the alignment in bytes the kernels need of it
struct SdcNamedArray {
  const char* name;
  const void* p;
  unsigned align;
};
// the names of v's arrays of that alignment (0: of all of them), `sep` between them and `last` in front of the last one
static inline std::string sdc_array_names(const std::vector<SdcNamedArray>& v, const unsigned align, const char* sep, const char* last) {
  std::string s, tail;
  for (const SdcNamedArray& x : v)
    if (!align || x.align == align) {
      if (!tail.empty()) s += (s.empty() ? "" : sep) + tail;
      tail = x.name;
    }
  return s.empty() ? tail : s + last + tail;
}
// What both calls refuse about their own arrays, each list in its signature's order: `plan`, the planner's (all required, 8-byte or
// dword aligned), and `opt`, the statistics' (given together or not at all, 16-byte or dword aligned)
static inline SdcMsg sdc_mpc_arrays_refused(const std::string& w, const std::vector<SdcNamedArray>& plan, const std::vector<SdcNamedArray>& opt) {
  uintptr_t bits[2][17] = {};      // the addresses OR-ed together, by list and alignment
  for (const SdcNamedArray& x : plan) bits[0][x.align] |= reinterpret_cast<uintptr_t>(x.p);
  for (const SdcNamedArray& x : opt) bits[1][x.align] |= reinterpret_cast<uintptr_t>(x.p);
  for (const SdcNamedArray& x : plan)
    if (!x.p) return w + "null array (" + sdc_array_names(plan, 0, ", ", " and ") + " are required)";
  if (bits[0][8] & 7u) return w + sdc_array_names(plan, 8, " / ", " / ") + " not 8-byte aligned";
  if (bits[0][4] & 3u) return w + sdc_array_names(plan, 4, " / ", " / ") + " not dword-aligned";
  for (const SdcNamedArray& x : opt)
    if ((x.p == nullptr) != (opt[0].p == nullptr)) return w + sdc_array_names(opt, 0, ", ", " and ") + " are given together or not at all";
  if (bits[1][16] & 15u) return w + sdc_array_names(opt, 16, " / ", " / ") + " not 16-byte aligned";
  if (bits[1][4] & 3u) return w + sdc_array_names(opt, 4, " / ", " / ") + " not dword-aligned";
  return std::nullopt;
}

// the longest planned decision of a call of n_steps that starts `left` steps before the episode's end: the first one (the horizon only
// shrinks towards the episode's end); 0: every decision idles
static inline int sdc_mpc_longest(const int H, const int warm_start, const int auto_reset, const int resume_steps, const int left, const int n_steps) {
  int k_max = 0;
  SdcMpcSchedule S(H, warm_start, auto_reset, resume_steps);
  for (int t = 0; t < n_steps; t++) k_max = std::max(k_max, S.next(left - t).steps);
  return k_max;
}
// ... and what the forecast refuses of it: the last refusal of both calls (m: the loop's fields of either parameter struct)
template <class Params>
static inline SdcMsg sdc_mpc_reach_refused(const std::string& w, const SdcCallFacts& f, const Params& m, const int left, const int n_steps,
                                    int& k_max) {
  k_max = sdc_mpc_longest(m.horizon, m.warm_start, f.auto_reset ? 1 : 0, m.resume ? m.resume_steps : 0, left, n_steps);
  if (k_max > 0) return sdc_forecast_refused(w, f, k_max);
  return std::nullopt;
}

// obj: the objective with the defaults filled in; k_max: the longest planned decision (sdc_mpc_longest)
static inline SdcMsg sdc_rollout_cem_stats_refused(const SdcCallFacts& f, const int n_steps, const sdc_mpc_params* mpc,
                                            const sdc_plan_objective* objective, const int accumulate, const SdcStatsArrays& a,
                                            const int32_t* plan_counts, const double* plan_sums, const double* probs, const int32_t* best_seq,
                                            const double* best_score, const int32_t* best_action, const int32_t* cand,
                                            const double* cand_score, sdc_plan_objective& obj, int& k_max) {
  static const std::string w = "sdc_rollout_cem_stats: ";
  if (SdcMsg m = sdc_stats_common_refused(w, f, n_steps, accumulate, a)) return m;
  if (!mpc) return w + "null mpc";
  if (SdcMsg m = sdc_mpc_loop_refused(w, mpc->horizon, mpc->warm_start, mpc->resume, mpc->resume_steps, mpc->idle_action)) return m;
  if (SdcMsg m = sdc_cem_params_refused(w, mpc->cem)) return m;
  if (SdcMsg m = sdc_mpc_arrays_refused(w,
                                        {{"probs", probs, 8}, {"best_seq", best_seq, 4}, {"best_score", best_score, 8},
                                         {"best_action", best_action, 4}, {"cand", cand, 4}, {"cand_score", cand_score, 8}},
                                        {{"plan_counts", plan_counts, 4}, {"plan_sums", plan_sums, 16}}))
    return m;
  if (SdcMsg m = sdc_plan_objective_refused(w, objective, obj)) return m;
  if (SdcMsg m = sdc_stats_past_end_refused(w, n_steps, f.left)) return m;
  return sdc_mpc_reach_refused(w, f, *mpc, f.left, n_steps, k_max);
}

// (sync_first: behind the sync every replica stands where its group's first env stands, so the episode's end is the first envs')
static inline SdcMsg sdc_rollout_cem_groups_stats_refused(const SdcCallFacts& f, const int n_steps, const sdc_mpc_group_params* mpc,
                                                   const sdc_plan_objective* objective, const int accumulate, const SdcStatsArrays& a,
                                                   const int32_t* plan_counts, const double* plan_sums, const int32_t* diverged,
                                                   const double* probs, const int32_t* best_seq, const double* best_score,
                                                   const int32_t* best_action, const int32_t* step_actions, const int32_t* cand,
                                                   const double* cand_score, sdc_plan_objective& obj, int& k_max) {
  static const std::string w = "sdc_rollout_cem_groups_stats: ";
  if (SdcMsg m = sdc_stats_common_refused(w, f, n_steps, accumulate, a)) return m;
  if (!mpc) return w + "null mpc";
  const sdc_mpc_group_params& p = *mpc;
  if (SdcMsg m = sdc_mpc_loop_refused(w, p.horizon, p.warm_start, p.resume, p.resume_steps, p.idle_action)) return m;
  if (p.sync_first != 0 && p.sync_first != 1) return w + "sync_first = " + std::to_string(p.sync_first) + " outside {0, 1}";
  if (p.sync_first && p.resume)
    return w + "sync_first with resume (behind the sync the first planned decision starts fresh: nothing can be resumed)";
  if (SdcMsg m = sdc_cem_group_params_refused(w, f.n_envs, p.cem)) return m;
  if (SdcMsg m = sdc_mpc_arrays_refused(w,
                                        {{"probs", probs, 8}, {"best_seq", best_seq, 4}, {"best_score", best_score, 8},
                                         {"best_action", best_action, 4}, {"step_actions", step_actions, 4}, {"cand", cand, 4},
                                         {"cand_score", cand_score, 8}},
                                        {{"plan_counts", plan_counts, 4}, {"plan_sums", plan_sums, 16}, {"diverged", diverged, 4}}))
    return m;
  if (SdcMsg m = sdc_plan_objective_refused(w, objective, obj)) return m;
  const int R = p.cem.group_size;
  int left = f.left;      // (the steps the episode has left at the first decision)
  if (p.sync_first) {
    int most = 0;
    for (int e = 0; e < f.n_envs; e += R) most = std::max(most, f.mirror->t_rel(e));
    left = f.episode_steps - most;
  }
  if (SdcMsg m = sdc_stats_past_end_refused(w, n_steps, left)) return m;
  if (!p.sync_first)
    if (SdcMsg m = sdc_groups_out_of_step_refused(w, f, R)) return m;
  return sdc_mpc_reach_refused(w, f, p, left, n_steps, k_max);
}
