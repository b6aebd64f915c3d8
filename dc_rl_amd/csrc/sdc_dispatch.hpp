// sdc_dispatch.hpp -- WHICH KERNEL a stepping call lands on: the whole decision of sdc_step, sdc_rollout and sdc_rollout_actor as pure
// functions of a few facts about the handle and the call, and the table of the kernels behind each answer.
//
// Plain C++17: no HIP, no sdc_handle -- a host compiler alone builds it (tests/test_step_dispatch.py holds it to the documented rules
// without a GPU; tests/test_gpu_kernel_reach.py holds the library to the same tables on the device).  sdc_capi.hip fills SdcStepFacts
// (step_facts), asks for the path and launches what sdc_kernel_of names: nothing else decides.
//
// Five single-step kernels and five multi-step ones give the same results to the bit (DESIGN.md section 4.16 has this file as a table):
//   GENERAL   sdc_dynamics_kernel / sdc_rollout_kernel: any batch, two envs per wavefront;
//   PAIR      THE COMMON CASE (below), two envs per wavefront: sdc_dynamics_fast_kernel / sdc_rollout_fast_kernel / sdc_rollout_actor_kernel;
//   QUAD      ... four envs per wavefront, for batches large enough for that mapping to pay: sdc_*_quad_kernel;
//   WIDE      one LANE per env (sdc_wide.hip), single steps of the largest batches, the common case of <= 8 rack classes;
//   WIDE_GEN  ... its general form: several configs, rule-based policies, other dc / battery rewards.
#pragma once

#include "../../include/sustaindc_hip.h"
#include "sdc_tuning.hpp"

// ---- thresholds (measured on the MI355X: 1024 SIMDs; tools/step_scan.py) ------------------------------------------------------------
// Four envs per wavefront pay when a SIMD holds more than one such wavefront, or nothing overlaps its waits: single steps are faster
// with four from ~6 700 envs on (6144: 16.3 us with two, 16.7 with four; 7168: 21.7 / 18.3); the multi-step kernels (sdc_rollout,
// sdc_rollout_actor), whose two-env form keeps two wavefronts per SIMD and needs a second round above 4096 envs, from any batch above
// 4096 (5120 envs: rollout 17.7 / 14.0 us per step, closed loop 28.2 / 19.7).
#ifndef SDC_QUAD_MIN_ENVS_STEP
// (round 4: 5 632 envs = 704 env-pair workgroups = 2.75 dispatch rounds is the last size at which two envs per wavefront win --
// 12.6 against 13.1 us per step; 6 144 envs: 16.5 against 13.3, the third round full and the spare sweep wavefronts pushing 128 env
// wavefronts into a fourth)
#define SDC_QUAD_MIN_ENVS_STEP 5636
#endif
#ifndef SDC_QUAD_MIN_ENVS_LOOP
#define SDC_QUAD_MIN_ENVS_LOOP 4100
#endif
#ifndef SDC_WIDE_MIN_ENVS
// (measured, us per step with the episode boundary inside, lane per env / four per wavefront, round 6 -- after the record's one-line
// layout and the kernel-argument touch: 6 144 envs 13.74 / 13.40, 7 168: 14.02 / 13.69, 7 680: 14.16 / 14.34, 8 192: 14.25 / 14.47,
// 8 704: 14.63 / 15.52, 12 288: 15.6 / 21.4, 16 384: 16.5 / 24.8, 32 768: 23.6 / 40.5, 65 536: 42.7 / 73.4; round 5's crossover was 9 216)
#define SDC_WIDE_MIN_ENVS 7680
#endif
#ifndef SDC_WIDE_ROLLOUT_MIN_ENVS
// sdc_rollout: K single-step launches of the lane-per-env kernel from here, below it one K-step launch (a MULTI-STEP launch of four envs
// per wavefront has no launch boundary between its steps: it stays ahead of K lane-per-env launches up to here -- 8 192 envs: 11.6
// against 14.3 us per step, 12 288: 15.4 / 15.6, 16 384: 23.4 / 17.4)
#define SDC_WIDE_ROLLOUT_MIN_ENVS 12288
#endif
// the history ring's slot-major mirror exists from this many envs: sdc_device.hpp SDC_HIST_MIRROR_MIN_ENVS, which the lane-per-env kernel
// reads (measured there; sdc_capi.hip asserts that the two are one number)
constexpr int SDC_DISPATCH_HIST_MIRROR_MIN_ENVS = 49152;

// ---- debug_flags (include/sustaindc_hip.h SDC_DEBUG_*), by what they mean HERE --------------------------------------------------------
// the diagnostics of the measurement bits live in the general kernels only; a measurement build (-DSDC_FAST_DEBUG=1) keeps the clock
// stamps in the two-envs-per-wavefront common-case kernels as well (the four-env and lane-per-env kernels never have them)
constexpr int SDC_DEBUG_IN_PAIR_KERNELS = SDC_FAST_DEBUG ? (SDC_DEBUG_PHASES | SDC_DEBUG_STAMPS | SDC_DEBUG_RECORD_WAIT | SDC_DEBUG_HW_ID) : 0;
constexpr int SDC_DEBUG_MEASUREMENT = SDC_DEBUG_WHY_REBUILD | SDC_DEBUG_PHASES | SDC_DEBUG_STAMPS | SDC_DEBUG_RECORD_WAIT | SDC_DEBUG_HW_ID;
// ANY OF THESE -> THE GENERAL KERNEL: the override that asks for it, the measurement modes, the test hook that lives in it
constexpr int SDC_DEBUG_TO_GENERAL =
    SDC_DEBUG_GENERAL | SDC_DEBUG_BOUND_REPAIR | (SDC_DEBUG_MEASUREMENT & ~SDC_DEBUG_IN_PAIR_KERNELS);
// ... and so does a bit that has no name (nobody knows what it asks for: the kernel that can do everything)
constexpr int SDC_DEBUG_NAMED = SDC_DEBUG_VERIFY | SDC_DEBUG_MEASUREMENT | SDC_DEBUG_STEP_NO_ENV | SDC_DEBUG_GENERAL | SDC_DEBUG_PAIR |
                                SDC_DEBUG_QUAD | SDC_DEBUG_WIDE | SDC_DEBUG_WIDE_OFF | SDC_DEBUG_BOUND_REPAIR | SDC_PLAN_DEBUG_TWO_STEPS;
// (SDC_DEBUG_VERIFY is a launch of its own behind the step, SDC_DEBUG_STEP_NO_ENV is sdc_create's: neither touches the choice.  The
// mapping overrides -- PAIR, QUAD, WIDE, WIDE_OFF -- are named where they act, below)

// ---- what the decision depends on -------------------------------------------------------------------------------------------------
struct SdcStepFacts {
  // the handle's side
  int n_envs, n_cfg;                  // batch size; data-centre configs
  int racks_cfg0, rack_cls_cfg0;      // config 0: racks; rack classes (0: more than the lane-per-env kernel's common form holds)
  int racks_max;                      // several configs: the largest rack count in use ...
  bool prm_env_ok;                    // ... and every env has its own copy of its config's scalars
  bool wide_gen_ok;                   // the batch's configs qualify for the lane-per-env kernel's general form
  bool has_qcum_t, has_feat;          // the queue table's time-major mirror / the feature rows are allocated
  int n_feat_host;                    // envs whose episode has valid feature rows
  int rel_hint;                       // the episode step all envs are at (< 0: not in lock-step)
  int policy[3], reward_method[3];    // per agent slot
  int debug_flags;                    // SdcDev's (without SDC_PLAN_DEBUG_TWO_STEPS)
  // the call's side
  bool actions, share_obs, info, actions_out;     // the array was given
  bool timed;                         // a profiled sdc_step
  bool rows_al16;                     // obs, share_obs, info and final_obs start on 16-byte boundaries
  bool actions_out_al4;               // actions_out starts on a dword boundary
};

enum SdcStepPath { SDC_PATH_GENERAL, SDC_PATH_PAIR, SDC_PATH_QUAD, SDC_PATH_WIDE, SDC_PATH_WIDE_GEN };

// ---- the conditions, each written once -----------------------------------------------------------------------------------------------
inline bool sdc_all_policies(const int policy[3]) {
  return policy[0] != SDC_POLICY_EXTERNAL && policy[1] != SDC_POLICY_EXTERNAL && policy[2] != SDC_POLICY_EXTERNAL;
}
// what EVERY specialised kernel needs: all envs in lock-step with valid feature rows, every output array present, no profiling, an
// even number of envs, no flag that asks for the general kernel
inline bool sdc_specialised_ok(const SdcStepFacts& f) {
  const bool to_general = (f.debug_flags & SDC_DEBUG_TO_GENERAL) != 0 || (f.debug_flags & ~SDC_DEBUG_NAMED) != 0;
  return f.rel_hint >= 0 && f.has_feat && f.n_feat_host == f.n_envs && f.share_obs && f.info && !f.timed && (f.n_envs & 1) == 0 &&
         !to_general;
}
// THE COMMON CASE, for which the step / rollout kernels exist in a specialised form (sdc_pairstep.hpp, template FAST): the above, <= 32
// racks (one pass; several configs: every env's own copy of the scalars), the caller's actions on all three slots, the default rewards
inline bool sdc_common_case(const SdcStepFacts& f) {
  const bool racks_ok = f.n_cfg == 1 ? (f.racks_cfg0 > 0 && f.racks_cfg0 <= 32) : (f.prm_env_ok && f.racks_max <= 32);
  return sdc_specialised_ok(f) && racks_ok && f.actions && f.policy[0] == SDC_POLICY_EXTERNAL && f.policy[1] == SDC_POLICY_EXTERNAL &&
         f.policy[2] == SDC_POLICY_EXTERNAL && f.reward_method[0] == SDC_REWARD_DEFAULT && f.reward_method[1] == SDC_REWARD_DEFAULT &&
         f.reward_method[2] == SDC_REWARD_DEFAULT;
}
// four envs per wavefront, given the common case: a multiple of four envs of ONE config, from the threshold or when SDC_DEBUG_QUAD asks;
// SDC_DEBUG_PAIR (and a measurement build's stamps) keep two
inline bool sdc_quad_ok(const SdcStepFacts& f, const bool multi_step) {
  return (f.n_envs & 3) == 0 && f.n_cfg == 1 && (f.debug_flags & (SDC_DEBUG_PAIR | SDC_DEBUG_IN_PAIR_KERNELS)) == 0 &&
         (f.n_envs >= (multi_step ? SDC_QUAD_MIN_ENVS_LOOP : SDC_QUAD_MIN_ENVS_STEP) || (f.debug_flags & SDC_DEBUG_QUAD) != 0);
}
// which slot-major mirrors a batch gets (sdc_create allocates by this; the kernels that append keep what exists): the queue table's for
// every batch the lane-per-env kernel may serve -- a multiple of 64 envs, from SDC_WIDE_MIN_ENVS or when SDC_DEBUG_WIDE asks -- and the
// history ring's behind it for the largest of them
struct SdcWideMirrors {
  bool qcum_t, hist_t;
};
inline SdcWideMirrors sdc_wide_mirrors(const int n_envs, const int debug_flags) {
  const bool q = (n_envs & 63) == 0 && (n_envs >= SDC_WIDE_MIN_ENVS || (debug_flags & SDC_DEBUG_WIDE) != 0);
  return {q, q && n_envs >= SDC_DISPATCH_HIST_MIRROR_MIN_ENVS};
}
// the structural conditions of the lane-per-env kernel (either form): a batch with the queue table's mirror, no override for another
// mapping, whole-line stores through the workgroup's staging block (16-byte aligned output rows)
inline bool sdc_wide_structural(const SdcStepFacts& f) {
  constexpr int other_mapping = SDC_DEBUG_PAIR | SDC_DEBUG_QUAD | SDC_DEBUG_WIDE_OFF | SDC_DEBUG_IN_PAIR_KERNELS;
  return sdc_wide_mirrors(f.n_envs, f.debug_flags).qcum_t && f.has_qcum_t && (f.debug_flags & other_mapping) == 0 && f.rows_al16;
}
// ... its common-case form, given the common case: one config in <= 8 rack classes
inline bool sdc_wide_common(const SdcStepFacts& f) {
  return sdc_wide_structural(f) && f.n_cfg == 1 && f.racks_cfg0 <= 32 && f.rack_cls_cfg0 > 0;
}
// ... and its GENERAL form (sdc_wide.hip GEN): several configs (SdcWideCfg), rule-based policies on any slot, any reward function for
// the dc / battery agents.  The ls agent keeps default_ls_reward -- with another one the history is not appended to
// (utils/reward_creator.py:63), a mode the per-lane reward path does not have
inline bool sdc_wide_general(const SdcStepFacts& f) {
  return sdc_specialised_ok(f) && sdc_wide_structural(f) && f.wide_gen_ok && (f.actions || sdc_all_policies(f.policy)) &&
         f.reward_method[0] == SDC_REWARD_DEFAULT;
}

// ---- the three decisions, in priority order ------------------------------------------------------------------------------------------
inline SdcStepPath sdc_single_step_path(const SdcStepFacts& f) {
  const bool common = sdc_common_case(f);
  if (common && sdc_wide_common(f)) return SDC_PATH_WIDE;
  if (sdc_wide_general(f)) return SDC_PATH_WIDE_GEN;      // a large batch of SEVERAL configs, or with policies / other reward functions
  if (common && sdc_quad_ok(f, false)) return SDC_PATH_QUAD;
  if (common) return SDC_PATH_PAIR;
  return SDC_PATH_GENERAL;
}

// sdc_rollout (f.timed is false): `per_step` -- n_steps SINGLE-step launches of `path`'s kernel, the deferred re-centrings running
// between them as in sdc_step; else ONE n_steps launch of its multi-step kernel.  The lane-per-env kernel has no multi-step form: a batch
// it serves takes the per-step way from SDC_WIDE_ROLLOUT_MIN_ENVS envs (or when SDC_DEBUG_WIDE asks), its general form when the applied
// actions are wanted (only the general kernels write them).  (The slices of step k start k * N rows in: aligned like the arrays
// themselves for the batches that kernel takes, N % 64 == 0)
struct SdcRolloutPath {
  SdcStepPath path;
  bool per_step;
};
inline SdcRolloutPath sdc_rollout_path(const SdcStepFacts& f) {
  const bool common = sdc_common_case(f) && !f.actions_out;
  const bool roll_wide = f.n_envs >= SDC_WIDE_ROLLOUT_MIN_ENVS || (f.debug_flags & SDC_DEBUG_WIDE) != 0;
  if (roll_wide && common && sdc_wide_common(f)) return {SDC_PATH_WIDE, true};
  if (roll_wide && sdc_wide_general(f) && (!f.actions_out || f.actions_out_al4)) return {SDC_PATH_WIDE_GEN, true};
  if (common && sdc_quad_ok(f, true)) return {SDC_PATH_QUAD, false};
  if (common) return {SDC_PATH_PAIR, false};
  return {SDC_PATH_GENERAL, false};
}

// sdc_rollout_actor (f.actions is true: the actors supply them; f.timed false): the common case only, and not in verify mode (which
// checks single steps)
struct SdcActorPath {
  bool refused;
  SdcStepPath path;      // SDC_PATH_PAIR or SDC_PATH_QUAD
};
inline SdcActorPath sdc_actor_path(const SdcStepFacts& f) {
  if (!sdc_common_case(f) || (f.debug_flags & SDC_DEBUG_VERIFY) != 0) return {true, SDC_PATH_GENERAL};
  return {false, sdc_quad_ok(f, true) ? SDC_PATH_QUAD : SDC_PATH_PAIR};
}

// ---- the kernels behind the answers ------------------------------------------------------------------------------------------------
enum SdcLaunchKind { SDC_LAUNCH_SINGLE, SDC_LAUNCH_MULTI, SDC_LAUNCH_ACTOR };
// who serves the deferred window re-centrings of a launch: nobody (a multi-step launch re-centres inline), SdcDev::sweep_blocks
// workgroups of four wavefronts at the front of the grid (as sdc_create sized them), or the lane-per-env kernel's own workgroups of two
// wavefronts, a request per wavefront
enum SdcSweepKind { SDC_SWEEP_NONE, SDC_SWEEP_COOP, SDC_SWEEP_WIDE };
struct SdcKernelInfo {
  const char* name;        // nullptr: there is no such kernel
  int envs_per_block;      // envs per workgroup ...
  int waves_per_block;     // ... of this many wavefronts
  SdcSweepKind sweep;
};
// by SdcStepPath: the single-step kernels, the multi-step ones, the closed loop's (the lane-per-env kernel has single steps only, the
// closed loop the common case only)
constexpr SdcKernelInfo SDC_NO_KERNEL = {nullptr, 1, 0, SDC_SWEEP_NONE};
constexpr SdcKernelInfo SDC_SINGLE_KERNELS[5] = {{"sdc_dynamics_kernel", 2 * SDC_STEP_WPB, SDC_STEP_WPB, SDC_SWEEP_COOP},
                                                 {"sdc_dynamics_fast_kernel", 2 * SDC_STEP_WPB, SDC_STEP_WPB, SDC_SWEEP_COOP},
                                                 {"sdc_dynamics_quad_kernel", 4 * SDC_STEP_WPB, SDC_STEP_WPB, SDC_SWEEP_COOP},
                                                 {"sdc_dynamics_wide_kernel", 64, 2, SDC_SWEEP_WIDE},
                                                 {"sdc_dynamics_wide_gen_kernel", 64, 2, SDC_SWEEP_WIDE}};
constexpr SdcKernelInfo SDC_MULTI_KERNELS[3] = {{"sdc_rollout_kernel", 2 * SDC_STEP_WPB, SDC_STEP_WPB, SDC_SWEEP_NONE},
                                                {"sdc_rollout_fast_kernel", 2 * SDC_STEP_WPB, SDC_STEP_WPB, SDC_SWEEP_NONE},
                                                {"sdc_rollout_quad_kernel", 4 * SDC_STEP_WPB, SDC_STEP_WPB, SDC_SWEEP_NONE}};
constexpr SdcKernelInfo SDC_ACTOR_KERNELS[3] = {SDC_NO_KERNEL,
                                                {"sdc_rollout_actor_kernel", 2 * SDC_ACTOR_WPB, SDC_ACTOR_WPB, SDC_SWEEP_NONE},
                                                {"sdc_rollout_actor_quad_kernel", 4 * SDC_ACTOR_WPB, SDC_ACTOR_WPB, SDC_SWEEP_NONE}};
constexpr SdcKernelInfo sdc_kernel_of(const SdcStepPath path, const SdcLaunchKind kind) {
  if (kind == SDC_LAUNCH_SINGLE) return SDC_SINGLE_KERNELS[path];
  if (path > SDC_PATH_QUAD) return SDC_NO_KERNEL;
  return kind == SDC_LAUNCH_MULTI ? SDC_MULTI_KERNELS[path] : SDC_ACTOR_KERNELS[path];
}
// workgroups that carry envs (a launch's grid: these behind its sweep workgroups)
inline int sdc_env_blocks(const SdcKernelInfo& k, const int n_envs) { return (n_envs + k.envs_per_block - 1) / k.envs_per_block; }
