// sdc_capi.hip -- host side of the C-ABI declared in include/sustaindc_hip.h.
//
// Owns the device-resident state of N environments on one GPU and launches the kernels on the caller's stream:
// sdc_dynamics_kernel (one launch = one env-step of all N envs, rewards included), sdc_reset_kernel at episode
// boundaries, sdc_reward_verify_kernel only in verify mode.  No CPU fallback: every entry point fails with an
// error code when HIP reports one.
//
// WHAT A CALL REFUSES before it touches the device is not decided here: sdc_refusals.hpp holds one pure rule per entry point, call_facts
// below tells it what it may know of the handle, and refused() turns its message into -2 with sdc_last_error set.  The fail_msg calls
// left in this file need a HIP call's result (a device that is not there, an allocation or copy that failed) or come up while a kernel
// plan is built from a HIP header (a segment table that is full, a layout a plan does not know); the null checks of the small setters
// and getters and the parameter checks of sdc_setup.hpp are reported where they always were.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <memory>
#include <vector>

#include "sdc_device.hpp"
#include "sdc_dispatch.hpp"
#include "sdc_setup.hpp"
#include "sdc_kernels.hpp"
#include "sdc_mirror.hpp"
#include "sdc_actor.hpp"
#include "sdc_clone.hpp"
#include "sdc_snapshot.hpp"
#include "sdc_mark.hpp"
#include "sdc_cem.hpp"
#include "sdc_cem_groups.hpp"
#include "sdc_plan.hpp"
#include "sdc_plan_terms.hpp"
#include "sdc_critic.hpp"
#include "sdc_forecast.hpp"
#include "sdc_stats.hpp"
#include "sdc_policy_stats.hpp"
#include "sdc_onpolicy.hpp"
#include "sdc_actor_eval.hpp"
#include "sdc_actor_grad.hpp"
#include "sdc_critic_grad.hpp"
#include "sdc_optim_dev.hpp"
#include "sdc_minibatch_dev.hpp"
#include "sdc_pack_tables.hpp"
#include "sdc_nets.hpp"
#include "sdc_mpc.hpp"
#include "sdc_mpc_groups.hpp"
#include "sdc_mpc_schedule.hpp"
#include "sdc_refusals.hpp"

namespace {

thread_local std::string g_err;

int fail(const char* what, hipError_t e) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return -1;
}
int fail_msg(const std::string& m) {
  g_err = m;
  return -2;
}

// a rule's answer (sdc_refusals.hpp) -> 0 if it accepts, else -2 with the message set
int refused(const char* m) { return m ? fail_msg(m) : 0; }
int refused(const SdcMsg& m) { return m ? fail_msg(*m) : 0; }

#define HIP_TRY(expr)                          \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) return fail(#expr, _e); \
  } while (0)

struct Field {
  const char* name;
  void** ptr;      // plain per-env array (ptr != nullptr) ...
  size_t elem;     // ... of `elem` bytes per env,
  int rec_idx;     // or a field of a strided per-env record: first dword,
  int rec_dwords;  // width in dwords,
  int in_hdr = 0;  // 0: the 256-byte state record, 1: the 256-byte header
};

// The index entries of a launch (which envs, which rows) staged through pinned host memory into a device buffer: two slots of [N]
// entries of each (or of `slot_entries`, for what is not sized by the batch), used in turn and allocated together on first use.  A slot's event marks the launch that last read it; a call waits
// for it only before it overwrites that slot, i.e. for the call two back on the same stage (stage_acquire / stage_commit)
struct IdxStage {
  size_t entry_bytes;
  size_t slot_entries = 0;                // entries per slot (0: n_envs)
  unsigned char* dev = nullptr;           // [2][N]
  unsigned char* pin = nullptr;           // [2][N]
  hipEvent_t done[2] = {nullptr, nullptr};
  bool in_flight[2] = {false, false};
  bool ready = false;                     // all of the above or none
  int slot = 0;                           // the slot the next call fills
};

}  // namespace

struct sdc_handle {
  sdc_config cfg;
  SdcDev d;
  SdcHostMirror mirror;      // what the host knows of each env (sdc_mirror.hpp): every decision below is taken from it, none from the device
  int step_no = 3;           // steps launched (stamps the deferred window re-centrings; starts above the stamps of zeroed memory)
  int device;
  std::vector<void*> allocs;
  std::vector<Field> fields;
  // override staging (device)
  int* ovr_day = nullptr;
  int* ovr_hour = nullptr;
  double* ovr_ci_min = nullptr;
  double* ovr_ci_max = nullptr;
  double* ovr_t_min = nullptr;
  double* ovr_t_max = nullptr;
  // the three actor slots and the critic as the library holds a trainable network (sdc_nets.hpp SdcNet), filled when the first actor /
  // the first critic is set (nets_alloc); the closed loop's SdcActorDev [3] is actor[0]'s first pack
  SdcNet actor[3], critic;
  // closed loop (sdc_rollout_actor): the library's copy of the latest observations (what the first actions of a launch are chosen
  // from), allocated with the actors
  bool actor_lds_set = false;   // the closed-loop kernels' dynamic-LDS limit has been raised on this handle's device
  float* obs_latch = nullptr;
  bool latch_valid = false;
  const char* last_step_kernel = "";      // sdc_last_step_kernel
  // what sdc_setup.hpp derives: the sizes of sdc_create; host copies of the configs ([n_dc_configs]; zeros where dc_set is 0) and the
  // facts about them that sdc_dispatch.hpp asks for, behind the device's copies of their tables (rebuild_config_tables)
  SdcGeometry geo{};
  std::vector<SdcDcDev> dc_host;
  std::vector<unsigned char> dc_set;
  SdcConfigFacts facts;
  double* prm_env_dev = nullptr;          // [N][32] every env's own copy of its config's scalars (several configs: SdcDev::prm_env)
  double* prm_cfg_dev = nullptr;          // [n_dc_configs][32] each config's scalars: what a restore copies into prm_env
  SdcWideCfg* wcfg_dev = nullptr;         // [SDC_WIDE_MAX_CFG] the lane-per-env kernel's general form (sdc_wide.hip GEN): one per config
  bool tables_set = false, assigned = false, started = false;
  // optional per-kernel timing: the kernels stamp the device wall clock per workgroup into one slot per sampled step
  int prof = 0;       // sample every `prof`-th step (0 = off)
  long prof_tick = 0;
  unsigned long long* prof_buf = nullptr;  // [PROF_SLOTS][3][N][2]
  int prof_used = 0;
  std::vector<unsigned char> prof_has_reset;
  double wall_clock_khz = 100000.0;
  double acc_ms[5] = {0, 0, 0, 0, 0};      // dynamics, reward, reset, steps, resets
  // two stages, so that a clone never waits for a snapshot two calls back or the other way round: sdc_clone_envs' {src, dst} pairs, and
  // the {env, row, cfg_id, loc_id} of the snapshot / restore / mark / rewind calls
  IdxStage clone_stage{sizeof(int2)};
  IdxStage idx_stage{sizeof(int4)};
  // sdc_mark_envs / sdc_rewind_envs: which marks are alive is the mirror's; the index staging is idx_stage
  int mark_engine_id = 0;                 // this handle's id in the manifests it fills (given out by the first mark)
  // sdc_plan: the mark rows and the rollouts' output block (sdc_plan.hpp) are the handle's, grown on demand and freed with it; the
  // manifest of its mark; the discount table's staging
  unsigned char* plan_rows = nullptr;
  size_t plan_rows_bytes = 0;
  unsigned char* plan_out = nullptr;
  size_t plan_out_bytes = 0;
  std::vector<int32_t> plan_manifest;
  IdxStage plan_stage{sizeof(double), SDC_MARK_MAX_STEPS};
  // sdc_set_plan_terms: what the plan calls score with next to their objective (both counts 0: nothing set, every field 0)
  sdc_plan_terms plan_terms{};
  // sdc_set_plan_critic: the weight the plan calls give the critic's value of the horizon's last share_obs rows (0: off, nothing launched)
  double plan_critic_weight = 0.0;
  // sdc_set_plan_forecast: what the plan calls' rollouts believe the traces ahead are (every field 0: nothing set); the forecast
  // [n_steps + 2][N][4] of a plan call and the row bits its overlay replaces (sdc_forecast.hpp), grown on demand and freed with the handle
  sdc_plan_forecast plan_forecast{};
  unsigned char* plan_fc = nullptr;
  size_t plan_fc_bytes = 0;
  unsigned char* plan_saved = nullptr;
  size_t plan_saved_bytes = 0;
  // sdc_rollout_actor_stats: a chunk's actions and logits (sdc_policy_stats.hpp), grown on demand and freed with the handle
  unsigned char* policy_out = nullptr;
  size_t policy_out_bytes = 0;
  // sdc_gae: every env's sum and sum of squares of its advantages [N][2] (sdc_onpolicy.hpp), allocated on first use
  double* adv_part = nullptr;
  // sdc_ppo_terms: stage 1's partial statistics [SDC_PPO_MAX_BLOCKS][8], allocated on first use
  double* ppo_part = nullptr;
  // what only the critic has: the host record of its scale, shift and flags (what a get hands back that is no parameter); the ValueNorm
  // block (sdc_minibatch.hip), allocated with the critic -- "installed": sdc_set_value_norm has filled it and neither sdc_set_critic nor
  // sdc_set_critic_norm has been called since; while it is, the device's scale and shift are the block's, not critic_scale /
  // critic_shift (critic_norm_now answers).  Allocated on first use: the stage 1 statistics [SDC_PPO_MAX_BLOCKS][8] of sdc_value_loss /
  // sdc_value_loss_normed (their own, not sdc_ppo_terms' -- the two may run on different streams) and sdc_value_norm_update's partial
  // sums [SDC_VN_MAX_BLOCKS][2]
  float critic_scale = 1.0f, critic_shift = 0.0f;
  int critic_flags = 0;
  SdcValueNormDev* value_norm = nullptr;
  bool value_norm_installed = false;
  double* value_loss_part = nullptr;
  double* value_norm_part = nullptr;
};

namespace {

constexpr int PROF_SLOTS = 256;
// The step counter that stamps re-centring requests wraps at 3 * 2^22: a multiple of the 3 rotating request sets and of
// the 2^22 the header stamps are taken modulo, so set rotation and stamp ages stay continuous across the wrap (the one
// request in flight at the wrap misses its full-width result stamp and falls back to the inline sweep).
constexpr int STEP_WRAP = 3 << 22;
int next_step_no(int s, int by) {
  if (by == 0) return s > STEP_WRAP - 4096 ? s % 3 + 3 : s;     // a multi-step launch must not straddle the wrap
  s += by;
  return s >= STEP_WRAP ? s - STEP_WRAP : s;
}

template <typename T>
int dev_alloc(sdc_handle* h, T** p, size_t count, bool zero = true) {
  void* q = nullptr;
  HIP_TRY(hipMalloc(&q, count * sizeof(T)));
  if (zero) HIP_TRY(hipMemset(q, 0, count * sizeof(T)));
  h->allocs.push_back(q);
  *p = reinterpret_cast<T*>(q);
  return 0;
}

// ---- the networks (sdc_nets.hpp): every host path once, over an SdcNet; an entry point keeps its rule, its packs, what else it allocates
SdcCriticDev* critic_dev(const sdc_handle* h) { return h->critic.pack_as<SdcCriticDev>(SDC_CRITIC_PACK_VALUES); }      // (null before sdc_set_critic)
// first use of the `count` networks of one kind: their packed structs, master parameters, moments and state blocks (zeroed) and the
// kind's gather table `t` (sdc_pack_tables.hpp), then the records -- filled only once everything is there
template <int PACKS>
int nets_alloc(sdc_handle* h, SdcNet* nets, const int count, const int n_params, const int n_in, const int grad_max_blocks, const SdcPackTables<PACKS>& t) {
  SdcNet kind = sdc_net_kind(n_params, n_in, grad_max_blocks, PACKS, t.offset);
  for (int i = 0; i < PACKS; i++)
    if (dev_alloc(h, &kind.pack[i], (size_t)count * kind.pack_dwords[i]) != 0) return -1;
  for (float** p : {&kind.params, &kind.m, &kind.v})
    if (dev_alloc(h, p, (size_t)count * n_params) != 0) return -1;
  if (dev_alloc(h, &kind.state, count) != 0) return -1;
  int32_t* table = nullptr;
  if (dev_alloc(h, &table, t.table.size(), false) != 0) return -1;
  HIP_TRY(hipMemcpy(table, t.table.data(), t.table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  kind.table = table;
  sdc_nets_fill(nets, count, kind);
  return 0;
}
// a freshly set network: with the device idle, the host packs `packed` [n_packs] over its packed structs, a new optimiser (the master
// copy from the params struct's leading floats, the moments zeroed, the state block reset), and the host facts recorded
int net_install(SdcNet& n, const void* host_params, const void* const* packed, const int activation, const bool feature_norm) {
  const sdc_optim_state fresh{0, 1.0, 1.0, 0};
  const size_t bytes = (size_t)n.n_params * sizeof(float);
  HIP_TRY(hipDeviceSynchronize());
  for (int i = 0; i < n.n_packs; i++) HIP_TRY(hipMemcpy(n.pack[i], packed[i], (size_t)n.pack_dwords[i] * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(n.params, host_params, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(n.m, 0, bytes));
  HIP_TRY(hipMemset(n.v, 0, bytes));
  HIP_TRY(hipMemcpy(n.state, &fresh, sizeof(fresh), hipMemcpyHostToDevice));
  n.set = true, n.activation = activation, n.feature_norm = feature_norm;
  return 0;
}

// the episode's observation feature rows of the envs a reset kernel has just reset (sdc_features.hip); episodes too long
// for the kernel's LDS windows go without (the step then computes the features itself); the launch shape is sdc_geometry's
void launch_features(sdc_handle* h, const SdcDev& d, hipStream_t st) {
  const SdcGeometry& g = h->geo;
  if (!g.has_feat) return;
  hipLaunchKernelGGL(sdc_features_kernel, dim3(d.n_envs), dim3(SDC_WAVE * g.feat_waves), g.feat_lds_bytes, st, d, g.feat_use_sma);
}

// one field of every env's record (256-byte state record, or 256-byte header) <-> a dense host array
int rec_put(sdc_handle* h, int idx, int dwords, const void* host, int in_hdr = 0) {
  unsigned* base = in_hdr ? h->d.hdr : h->d.rec;
  const size_t pitch = sizeof(unsigned) * (in_hdr ? SDC_HDR_DWORDS : SDC_REC_DWORDS);
  HIP_TRY(hipMemcpy2D(base + idx, pitch, host, sizeof(unsigned) * dwords, sizeof(unsigned) * dwords,
                      (size_t)h->cfg.n_envs, hipMemcpyHostToDevice));
  return 0;
}
int rec_get(sdc_handle* h, int idx, int dwords, void* host, int in_hdr = 0) {
  const unsigned* base = in_hdr ? h->d.hdr : h->d.rec;
  const size_t pitch = sizeof(unsigned) * (in_hdr ? SDC_HDR_DWORDS : SDC_REC_DWORDS);
  HIP_TRY(hipMemcpy2D(host, sizeof(unsigned) * dwords, base + idx, pitch, sizeof(unsigned) * dwords,
                      (size_t)h->cfg.n_envs, hipMemcpyDeviceToHost));
  return 0;
}

// the episode's precomputed observation rows follow the traces, the env's location and its weather windows
int invalidate_features(sdc_handle* h) {
  std::vector<unsigned> z((size_t)h->cfg.n_envs, 0u);
  h->mirror.features_invalidated();
  return rec_put(h, R_FEAT_OK, 1, z.data());
}
// WHICH KERNEL a stepping call lands on is decided in sdc_dispatch.hpp, from these facts about the handle and the call (`some_actions`:
// the caller's array, or the actors' choices for the closed loop) -- host fields, the mirror's two summaries and pointer bits, nothing per env
SdcStepFacts step_facts(const sdc_handle* h, const bool some_actions, const float* obs, const float* share_obs, const float* info,
                        const float* final_obs, const int32_t* actions_out, const bool timed) {
  const auto aligned = [](const void* p, const uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; };
  const SdcDev& d = h->d;
  SdcStepFacts f;
  f.n_envs = h->cfg.n_envs;
  f.n_cfg = d.n_cfg;
  f.racks_cfg0 = h->facts.racks_cfg0;
  f.rack_cls_cfg0 = h->facts.rack_cls_cfg0;
  f.racks_max = h->facts.racks_max;
  f.prm_env_ok = h->facts.prm_env_ok;
  f.wide_gen_ok = h->facts.wide_gen_ok;
  f.has_qcum_t = h->geo.mirrors.qcum_t;
  f.has_feat = h->geo.has_feat;
  f.n_feat_host = h->mirror.n_feat();
  f.rel_hint = h->mirror.rel_hint();
  for (int a = 0; a < 3; a++) {
    f.policy[a] = d.policy[a];
    f.reward_method[a] = d.reward_method[a];
  }
  f.debug_flags = d.debug_flags;
  f.actions = some_actions;
  f.share_obs = share_obs != nullptr;
  f.info = info != nullptr;
  f.actions_out = actions_out != nullptr;
  f.timed = timed;
  f.rows_al16 = aligned(obs, 16) && aligned(share_obs, 16) && aligned(info, 16) && aligned(final_obs, 16);
  f.actions_out_al4 = aligned(actions_out, 4);
  return f;
}
static_assert(SDC_DISPATCH_HIST_MIRROR_MIN_ENVS == SDC_HIST_MIRROR_MIN_ENVS, "sdc_wide_mirrors and the lane-per-env kernel: one threshold");
static_assert(sdc_kernel_of(SDC_PATH_WIDE, SDC_LAUNCH_SINGLE).envs_per_block == SDC_WAVE, "the lane-per-env kernel: a wavefront of envs per workgroup");

// a clone or a restore has moved assignments: the largest rack count in use, which the common case (sdc_dispatch.hpp) asks of a batch
// of several configs
void refresh_racks_max(sdc_handle* h) {
  if (h->facts.prm_env_ok) h->facts.racks_max = sdc_racks_max(h->dc_host.data(), h->mirror.cfg_ids(), h->cfg.n_envs);
}

// the configs or the assignment have changed: derive the batch's tables and facts again (sdc_setup.hpp) and upload the tables.  A fact
// that rests on a table holds once the table is on the device
int rebuild_config_tables(sdc_handle* h) {
  SdcDev& d = h->d;
  const int N = h->cfg.n_envs, C = h->cfg.n_dc_configs;
  const SdcConfigTables t = sdc_config_tables(h->dc_host.data(), h->dc_set.data(), C, h->mirror.cfg_ids(), N);
  h->facts = SdcConfigFacts{};
  d.prm_env = nullptr;
  d.wcfg = nullptr;
  if (t.facts.prm_env_ok) {
    if (!h->prm_env_dev && dev_alloc(h, &h->prm_env_dev, (size_t)N * SDC_PRM_ROW) != 0) return -1;
    HIP_TRY(hipMemcpy(h->prm_env_dev, t.prm_env.data(), sizeof(double) * t.prm_env.size(), hipMemcpyHostToDevice));
    if (!h->prm_cfg_dev && dev_alloc(h, &h->prm_cfg_dev, (size_t)C * SDC_PRM_ROW) != 0) return -1;
    HIP_TRY(hipMemcpy(h->prm_cfg_dev, t.prm_cfg.data(), sizeof(double) * t.prm_cfg.size(), hipMemcpyHostToDevice));
    d.prm_env = h->prm_env_dev;
  }
  if (t.facts.wide_gen_ok) {
    if (!h->wcfg_dev && dev_alloc(h, &h->wcfg_dev, (size_t)SDC_WIDE_MAX_CFG) != 0) return -1;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->wcfg_dev, t.wide.data(), sizeof(SdcWideCfg) * t.wide.size(), hipMemcpyHostToDevice));
    d.wcfg = h->wcfg_dev;
    d.wide_max_cls = t.wide_max_cls;
    d.wide_max_racks4 = t.wide_max_racks4;
  }
  h->facts = t.facts;
  return 0;
}

// the reward state (rank windows, running sums) describes the ring contents: drop it when the ring is injected
int invalidate_trackers(sdc_handle* h) {
  std::vector<unsigned> z((size_t)h->cfg.n_envs, 0u);
  if (rec_put(h, H_VALID, 1, z.data(), 1)) return -1;
  return 0;
}

// keep the library's copy of the latest observations (closed loop only: no actor set, no copy)
int latch_obs(sdc_handle* h, const float* obs, hipStream_t st) {
  if (!h->obs_latch || !obs) return 0;
  HIP_TRY(hipMemcpyAsync(h->obs_latch, obs, sizeof(float) * (size_t)h->cfg.n_envs * SDC_OBS_OUT, hipMemcpyDeviceToDevice, st));
  h->latch_valid = true;
  return 0;
}

// the kernels behind sdc_dispatch.hpp's table, by SdcStepPath
using StepKernel = void (*)(SdcDev, int, const int32_t*, float*, float*, unsigned char*, float*, float*, float*);
using RolloutKernel = void (*)(SdcDev, int, int, const int32_t*, float*, float*, unsigned char*, float*, float*, float*);
constexpr StepKernel STEP_KERNELS[5] = {sdc_dynamics_kernel, sdc_dynamics_fast_kernel, sdc_dynamics_quad_kernel, sdc_dynamics_wide_kernel,
                                        sdc_dynamics_wide_gen_kernel};
constexpr RolloutKernel ROLLOUT_KERNELS[3] = {sdc_rollout_kernel, sdc_rollout_fast_kernel, sdc_rollout_quad_kernel};

// one single-step launch of `path`'s kernel: its sweep workgroups at the front of the grid, the env workgroups behind them
void launch_step(sdc_handle* h, SdcDev& d, const SdcStepPath path, const int rel, const int32_t* actions, float* obs, float* share_obs,
                 unsigned char* done, float* info, float* final_obs, float* rew, hipStream_t st) {
  const SdcKernelInfo k = sdc_kernel_of(path, SDC_LAUNCH_SINGLE);
  if (k.sweep == SDC_SWEEP_WIDE) d.sweep_blocks = std::min(d.rq_max, 256) / 2;     // (two wavefronts each, a request per wavefront)
  h->last_step_kernel = k.name;
  hipLaunchKernelGGL(STEP_KERNELS[path], dim3(d.sweep_blocks + sdc_env_blocks(k, h->cfg.n_envs)), dim3(SDC_WAVE * k.waves_per_block), 0, st,
                     d, rel, actions, obs, share_obs, done, info, final_obs, rew);
}
// ... and one launch of its multi-step kernel (no sweep workgroups: it re-centres inline)
void launch_rollout(sdc_handle* h, const SdcDev& d, const SdcStepPath path, const int n_steps, const int32_t* actions, float* obs,
                    float* share_obs, unsigned char* done, float* info, float* final_obs, float* rew, hipStream_t st) {
  const SdcKernelInfo k = sdc_kernel_of(path, SDC_LAUNCH_MULTI);
  h->last_step_kernel = k.name;
  hipLaunchKernelGGL(ROLLOUT_KERNELS[path], dim3(sdc_env_blocks(k, h->cfg.n_envs)), dim3(SDC_WAVE * k.waves_per_block), 0, st, d, n_steps,
                     h->mirror.rel_hint(), actions, obs, share_obs, done, info, final_obs, rew);
}

// What every stepping call does behind its launch(es) of n_steps steps; obs_last / share_obs_last (may be NULL) are the LAST step's
// slices.  Episodes have a fixed length and every env advances one step per launched step, so the host knows from its mirror
// (sdc_mirror.hpp) when an env has finished -- no device read-back.  With auto_reset the finished envs are reset inside the call
// (harl/envs/env_wrappers.py:176-190): the last step's obs / share_obs receive the reset observation, final_obs keeps the pre-reset
// one.  `timed`: the launch was a profiled sdc_step.  The closed loop's copy of the latest observations is taken in every case
// (`latch_always`) or only after an auto-reset (sdc_rollout_actor: its kernel writes the copy itself)
int finish_launch(sdc_handle* h, SdcDev& d, const int n_steps, float* obs_last, float* share_obs_last, hipStream_t st, const bool timed,
                  const bool latch_always) {
  HIP_TRY(hipGetLastError());
  const int N = h->cfg.n_envs;
  bool was_reset = false;
  if (h->mirror.stepped(n_steps) && h->cfg.auto_reset) {      // at least one env just finished
    d.reset_mask = nullptr;
    if (timed) h->prof_has_reset[h->prof_used] = 1;
    hipLaunchKernelGGL(sdc_reset_kernel, dim3(N), dim3(SDC_WAVE), 0, st, d, 0, h->ovr_day, h->ovr_hour, h->ovr_ci_min, h->ovr_ci_max,
                       h->ovr_t_min, h->ovr_t_max, 1, obs_last, share_obs_last, nullptr, nullptr);
    launch_features(h, d, st);
    HIP_TRY(hipGetLastError());
    h->mirror.finished_envs_reset();
    was_reset = true;
  }
  if (timed) h->prof_used += 1;
  if (latch_always || was_reset) return latch_obs(h, obs_last, st) ? -1 : 0;
  return 0;
}

// ---- the env-copy calls' plumbing (clone, snapshot / restore, mark / rewind) ----------------------------------------------------------
// The pinned side of the slot this call fills.  Allocates on first use -- all staging resources or none: a failure part way leaves
// `ready` false, and the next call starts over from what is set -- and waits for the call two back if it may still be reading the slot
int stage_acquire(sdc_handle* h, IdxStage& S, void** pin) {
  const size_t slot_bytes = S.entry_bytes * (S.slot_entries ? S.slot_entries : (size_t)h->cfg.n_envs);
  if (!S.ready) {
    if (!S.dev && dev_alloc(h, &S.dev, 2 * slot_bytes, false) != 0) return -1;
    if (!S.pin) {
      void* q = nullptr;
      HIP_TRY(hipHostMalloc(&q, 2 * slot_bytes, hipHostMallocDefault));
      S.pin = static_cast<unsigned char*>(q);
    }
    for (int i = 0; i < 2; i++)
      if (!S.done[i]) {
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        S.done[i] = ev;
      }
    S.ready = true;
  }
  const int slot = S.slot;
  S.slot ^= 1;
  if (S.in_flight[slot]) {
    HIP_TRY(hipEventSynchronize(S.done[slot]));
    S.in_flight[slot] = false;
  }
  *pin = S.pin + (size_t)slot * slot_bytes;
  return 0;
}
// ... and its first n entries on their way: copied to the device, read by launch(the device side of the slot) -> hipError_t, and the
// slot in flight until that launch is done
template <typename Launch>
int stage_commit(sdc_handle* h, IdxStage& S, const size_t n, hipStream_t st, Launch launch) {
  const int slot = S.slot ^ 1;      // (the slot stage_acquire has just handed out)
  const size_t off = (size_t)slot * S.entry_bytes * (S.slot_entries ? S.slot_entries : (size_t)h->cfg.n_envs);
  HIP_TRY(hipMemcpyAsync(S.dev + off, S.pin + off, S.entry_bytes * n, hipMemcpyHostToDevice, st));
  HIP_TRY(launch(S.dev + off));
  HIP_TRY(hipEventRecord(S.done[slot], st));
  S.in_flight[slot] = true;
  return 0;
}
// both, for entries the caller has built elsewhere
template <typename Launch>
int stage_send(sdc_handle* h, IdxStage& S, const void* entries, const size_t n, hipStream_t st, Launch launch) {
  void* pin = nullptr;
  if (stage_acquire(h, S, &pin)) return -1;
  std::memcpy(pin, entries, S.entry_bytes * n);
  return stage_commit(h, S, n, st, launch);
}
void stage_destroy(IdxStage& S) {
  for (int i = 0; i < 2; i++) {
    if (S.in_flight[i]) (void)hipEventSynchronize(S.done[i]);
    if (S.done[i]) (void)hipEventDestroy(S.done[i]);
  }
  if (S.pin) (void)hipHostFree(S.pin);
}

// One env-major array joins the segment table of a copy plan (SdcClonePlan, SdcSnapPlan: the same fields) as a wide segment (16-byte
// units) or a narrow one (dwords).  Which, is the caller's rule:
//   SEG_DEMOTE (the clone): wide if pitch AND base are 16-byte aligned, else narrow -- any array can be copied;
//   SEG_BY_PITCH (the snapshot): by the pitch alone, because the row layout must not depend on a pointer; a wide array with a
//     misaligned base is refused, and so is a base that is not dword-aligned.
// -> false (and nothing added) if refused or the class's table is full
enum SegPolicy { SEG_DEMOTE, SEG_BY_PITCH };
template <typename Plan>
bool seg_add(Plan& P, const SegPolicy policy, void* base, const size_t pitch) {
  const uintptr_t b = reinterpret_cast<uintptr_t>(base);
  const bool wide = pitch % 16 == 0 && (policy == SEG_BY_PITCH || (b & 15u) == 0);
  if (policy == SEG_BY_PITCH && ((wide && (b & 15u) != 0) || (b & 3u) != 0)) return false;
  constexpr int max_wide = (int)(sizeof(P.wide) / sizeof(P.wide[0])), max_narrow = (int)(sizeof(P.narrow) / sizeof(P.narrow[0]));
  if (wide ? P.n_wide == max_wide : P.n_narrow == max_narrow) return false;
  int& count = wide ? P.n_wide : P.n_narrow;
  unsigned& units = wide ? P.wide_units : P.narrow_units;
  SdcSeg& g = wide ? P.wide[count] : P.narrow[count];
  g.base = static_cast<unsigned char*>(base);
  g.pitch = (unsigned)pitch;
  g.first = units;
  count += 1;
  units += (unsigned)(pitch / (wide ? 16 : 4));
  return true;
}

}  // namespace

extern "C" {

const char* sdc_last_error(void) { return g_err.c_str(); }
int sdc_version(void) { return SDC_ABI_VERSION; }

// FNV-1a over the checkpoint's raw layouts: the record's and the header's dword offsets and the ring's stride.  A re-laid-out
// record keeps its byte size, so the size check of sdc_set_state cannot tell an old checkpoint from a current one; this can.
static constexpr unsigned kStateLayout[] = {
    SDC_REC_DWORDS, SDC_HDR_DWORDS, SDC_HIST_STRIDE,
    R_CURSOR, R_TREL, R_DAY, R_HOURQ, R_QPOPPED, R_QCUM, R_QCUMT, R_QHEAD, R_QCUM_HM1, R_QCUMT_HM1, R_LAST_DELTA, R_CONSEC,
    R_SCALE, R_HIST_LEN, R_HIST_POS, R_FAULT, R_F64, R_STPT, R_BAT, R_HIST_REF, R_LAST_ROOM, R_CFG, R_LOC, R_TR_COUNT,
    R_EPISODE, R_CI_MIN, R_CI_DEN, R_DAY_LO, R_DAY_HI, R_FEAT_OK, R_T_MIN, R_T_DEN, R_END,
    H_N, H_QS2_LO, H_EOFF, H_QS1, H_RET, H_Q1, H_BU, H_BL, H_QC, H_Q3, H_WFIRST, H_WLAST, H_PEND, H_LAST_XNEW, H_LAST_XOLD,
    H_LAST_NPREV, H_QS2_HI, H_STICKY, H_KB, H_VALID, H_A1, H_A2,
    T_R0, T_HI, SDC_TRACK_DWORDS, SDC_WIN};
static constexpr uint32_t state_layout_hash() {
  uint32_t x = 2166136261u;
  for (unsigned v : kStateLayout)
    for (int b = 0; b < 4; b++) x = (x ^ ((v >> (8 * b)) & 0xFFu)) * 16777619u;
  return x;
}
uint32_t sdc_state_layout(void) { return state_layout_hash(); }

// WHAT A REFUSAL MAY KNOW OF THE HANDLE (sdc_refusals.hpp): host fields and the mirror's summaries, nothing per env.  stepping_facts:
// the few scalars sdc_step, sdc_rollout and sdc_rollout_actor read, and nothing else -- a step pays for no more; call_facts: all of it
// (the closed-loop rule's step facts are the caller's to add)
static void fill_stepping_facts(const sdc_handle* h, SdcSteppingFacts& f) {
  f.handle = true;
  f.started = h->started;
  f.left = h->mirror.steps_to_terminal();
  f.debug_flags = h->cfg.debug_flags;
  f.all_policies = sdc_all_policies(h->d.policy);
  for (int a = 0; a < 3; a++) {
    f.actor_set[a] = h->actor[a].set;
    f.actor_activation[a] = h->actor[a].activation;
  }
  f.latch_valid = h->latch_valid;
  f.critic_set = h->critic.set;
}
static SdcSteppingFacts stepping_facts(const sdc_handle* h) {
  SdcSteppingFacts f;
  if (h) fill_stepping_facts(h, f);
  return f;
}
static SdcCallFacts call_facts(const sdc_handle* h) {
  SdcCallFacts f;
  if (!h) return f;
  fill_stepping_facts(h, f);
  f.n_envs = h->cfg.n_envs;
  f.episode_steps = h->cfg.episode_steps;
  f.hist_cap = h->cfg.hist_cap;
  f.n_locations = h->cfg.n_locations;
  f.n_dc_configs = h->cfg.n_dc_configs;
  f.auto_reset = h->cfg.auto_reset;
  f.tables_set = h->tables_set;
  f.assigned = h->assigned;
  f.has_feat = h->d.feat != nullptr;
  f.state_layout = state_layout_hash();
  f.qstride = h->d.qstride;
  f.lw = h->d.lw;
  f.rec_dwords = SDC_REC_DWORDS;
  f.rec_cfg = R_CFG;
  f.mark_engine_id = h->mark_engine_id;
  f.forecast = h->plan_forecast;
  f.mirror = &h->mirror;
  return f;
}

int sdc_create(const sdc_config* cfg, sdc_handle** out) {
  if (!cfg || !out) return fail_msg("sdc_create: null argument");
  const SdcRefusal refusal = sdc_check_config(*cfg);      // (sdc_setup.hpp: every check that needs no device)
  if (refusal.msg && !refusal.after_device) return fail_msg(refusal.msg);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev) return fail_msg("sdc_create: no such HIP device");
  HIP_TRY(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail_msg(std::string("sdc_create: built for gfx950 (MI355X) only, device is ") + prop.gcnArchName);
  if (refusal.msg) return fail_msg(refusal.msg);

  sdc_handle* h = new sdc_handle();
  h->cfg = *cfg;
  const SdcGeometry& g = h->geo = sdc_geometry(*cfg);
  h->dc_host.assign((size_t)cfg->n_dc_configs, SdcDcDev{});      // (a config that is never set: zeros, like the device's copy)
  h->dc_set.assign((size_t)cfg->n_dc_configs, 0);
  if (cfg->debug_flags & SDC_DEBUG_STEP_NO_ENV)   // test hook (tests of the launch counter's wrap): start the counter where the environment says
    if (const char* t = std::getenv("SDC_TEST_STEP_NO")) h->step_no = std::atoi(t) % STEP_WRAP;
  h->device = cfg->device;
  SdcDev& d = h->d;
  std::memset(&d, 0, sizeof(d));
  const int N = cfg->n_envs;
  d.n_envs = N;
  d.episode_steps = cfg->episode_steps;
  d.hist_cap = cfg->hist_cap;
  d.queue_max = cfg->queue_max_len;
  d.rc_queue_max = 1.0 / (double)cfg->queue_max_len;
  d.rc_hist_cap = 1.0 / (double)cfg->hist_cap;
  d.queue_max_d = (double)cfg->queue_max_len;
  d.hist_cap_d = (double)cfg->hist_cap;
  d.table_len = SDC_TABLE_LEN;
  static_assert(SDC_TABLE_LEN % 8 == 0, "sdc_reset_kernel: a lane's 8 samples of the year's walk are all inside the table or all outside");
  d.lw = g.lw;
  d.qstride = g.qstride;
  d.max_roll_days = cfg->max_roll_days;
  d.debug_flags = cfg->debug_flags & ~SDC_PLAN_DEBUG_TWO_STEPS;      // (sdc_plan's test hook: read from h->cfg by that call alone)
  d.env_base = cfg->env_index_base;
  for (int a = 0; a < 3; a++) {
    d.reward_method[a] = cfg->reward_method[a];
    d.policy[a] = cfg->policy[a];
  }
  d.tr_limit = cfg->trim_and_respond_limit;
  d.actions_out = nullptr;
  d.seed = cfg->seed;
  d.noise_std = cfg->weather_noise_std;
  d.noise_weight = cfg->weather_noise_weight;

#define A(ptr, count)                                              \
  do {                                                             \
    if (dev_alloc(h, &(ptr), (size_t)(count)) != 0) {              \
      sdc_destroy(h);                                              \
      return -1;                                                   \
    }                                                              \
  } while (0)
  double *tabW, *tabC, *tabT, *tabWB, *hour_lut;
  SdcDcDev* dcp;
  A(tabW, (size_t)cfg->n_locations * SDC_TABLE_LEN);
  A(tabC, (size_t)cfg->n_locations * SDC_TABLE_LEN);
  A(tabT, (size_t)cfg->n_locations * SDC_TABLE_LEN);
  A(tabWB, (size_t)cfg->n_locations * SDC_TABLE_LEN);
  A(hour_lut, 96 * 2);
  A(dcp, cfg->n_dc_configs);
  d.tabW = tabW; d.tabC = tabC; d.tabT = tabT; d.tabWB = tabWB; d.hour_lut = hour_lut; d.dc = dcp; d.n_cfg = cfg->n_dc_configs;
  A(d.rec, (size_t)N * SDC_REC_DWORDS);
  A(d.qtab, (size_t)N * d.qstride);
  d.qcum_t = nullptr;
  d.hist_t = nullptr;
  if (g.mirrors.qcum_t) {      // (batches the lane-per-env kernel can serve)
    // ... and BEHIND it, in the same allocation, the history ring's slot-major mirror for the batches that get one (rows qstride ..
    // qstride + hist_cap of the same [row][N] array: the lane-per-env kernel addresses it from the pointer and the strides it holds anyway)
    const bool mirror = g.mirrors.hist_t;
    A(d.qcum_t, (size_t)N * ((size_t)d.qstride + (mirror ? (size_t)d.hist_cap : 0)));      // (zeroed by the allocation)
    if (mirror) {
      d.hist_t = d.qcum_t + (size_t)N * d.qstride;
      if (hipMemset(d.hist_t, 0xFF, sizeof(unsigned) * (size_t)N * d.hist_cap) != hipSuccess) {      // every slot empty
        sdc_destroy(h);
        return fail_msg("sdc_create: clearing the history rings' mirror failed");
      }
    }
  }
  A(d.t_win, (size_t)N * d.lw);
  A(d.wb_win, (size_t)N * d.lw);
  A(d.hist, (size_t)N * SDC_HIST_STRIDE);
  if (hipMemset(d.hist, 0xFF, sizeof(unsigned) * (size_t)N * SDC_HIST_STRIDE) != hipSuccess) {  // every slot empty
    sdc_destroy(h);
    return fail_msg("sdc_create: clearing the history rings failed");
  }
  A(d.hdr, (size_t)N * SDC_HDR_DWORDS);
  A(d.qwin, (size_t)N * (4 * SDC_WIN));
  d.feat = nullptr;
  if (g.has_feat) A(d.feat, (size_t)N * (size_t)(cfg->episode_steps + 1) * SDC_FEAT_ROW);
  A(d.rq_count, 4);
  d.rq_max = g.rq_max;      // deferred re-centring capacity by batch size
  d.sweep_blocks = g.sweep_blocks;
  A(d.rq, 3 * (size_t)d.rq_max);
  A(d.rs, 3 * (size_t)d.rq_max);
  A(d.reset_mask, N);
  A(h->ovr_day, N); A(h->ovr_hour, N);
  A(h->ovr_ci_min, N); A(h->ovr_ci_max, N); A(h->ovr_t_min, N); A(h->ovr_t_max, N);
#undef A

  // hour LUT: utils/managers.py:66-88 sc_obs -- round(hour/24, 3) * 2pi -> cos/sin * 0.5 + 0.5
  {
    double lut[192];
    const double two_pi = 3.141592653589793 * 2;
    for (int q = 0; q < 96; q++) {
      const double hour = q * 0.25;
      const double nh = (std::rint((hour / 24) * 1000.0) / 1000.0) * two_pi;
      lut[2 * q] = std::cos(nh) * 0.5 + 0.5;
      lut[2 * q + 1] = std::sin(nh) * 0.5 + 0.5;
    }
    if (hipMemcpy(hour_lut, lut, sizeof(lut), hipMemcpyHostToDevice) != hipSuccess) {
      sdc_destroy(h);
      return fail_msg("sdc_create: hour LUT upload failed");
    }
  }
  h->mirror = SdcHostMirror(N, cfg->episode_steps, g.has_feat);      // every env "finished": a reset is required before stepping
  h->fields = {
      {"cursor", nullptr, 4, R_CURSOR, 1}, {"t_rel", nullptr, 4, R_TREL, 1}, {"day", nullptr, 4, R_DAY, 1},
      {"hourq", nullptr, 4, R_HOURQ, 1}, {"q_popped", nullptr, 4, R_QPOPPED, 1}, {"q_cum", nullptr, 4, R_QCUM, 1},
      {"q_cumT", nullptr, 4, R_QCUMT, 1}, {"q_head", nullptr, 4, R_QHEAD, 1}, {"q_cum_hm1", nullptr, 4, R_QCUM_HM1, 1},
      {"q_cumT_hm1", nullptr, 4, R_QCUMT_HM1, 1}, {"last_delta", nullptr, 4, R_LAST_DELTA, 1},
      {"consecutive", nullptr, 4, R_CONSEC, 1}, {"scale", nullptr, 4, R_SCALE, 1}, {"hist_len", nullptr, 4, R_HIST_LEN, 1},
      {"hist_pos", nullptr, 4, R_HIST_POS, 1}, {"episode", nullptr, 4, R_EPISODE, 1}, {"fault", nullptr, 4, R_FAULT, 1},
      {"loc_id", nullptr, 4, R_LOC, 1}, {"cfg_id", nullptr, 4, R_CFG, 1}, {"day_lo", nullptr, 4, R_DAY_LO, 1},
      {"day_hi", nullptr, 4, R_DAY_HI, 1},
      {"stpt", nullptr, 8, R_STPT, 2}, {"bat_load", nullptr, 8, R_BAT, 2}, {"ci_min", nullptr, 8, R_CI_MIN, 2},
      {"ci_den", nullptr, 8, R_CI_DEN, 2}, {"t_min", nullptr, 8, R_T_MIN, 2}, {"t_den", nullptr, 8, R_T_DEN, 2},
      {"hist_ref", nullptr, 8, R_HIST_REF, 2},
      {"record", (void**)&d.rec, 4 * SDC_REC_DWORDS, 0, 0},
      {"hist", (void**)&d.hist, sizeof(unsigned) * SDC_HIST_STRIDE, 0, 0},
      {"hist_n", nullptr, 4, H_N, 1, 1}, {"ep_return", nullptr, 24, H_RET, 6, 1},
      {"order_stat_sticky", nullptr, 4, H_STICKY, 1, 1},
      {"header", (void**)&d.hdr, 4 * SDC_HDR_DWORDS, 0, 0},
      {"qwin", (void**)&d.qwin, 4 * 4 * SDC_WIN, 0, 0},
      {"t_win", (void**)&d.t_win, sizeof(double) * (size_t)d.lw, 0, 0},
      {"wb_win", (void**)&d.wb_win, sizeof(double) * (size_t)d.lw, 0, 0},
      {"qtab", (void**)&d.qtab, sizeof(uint2) * (size_t)d.qstride, 0, 0},
      // READ-ONLY (sdc_get_state alone; refused where the batch has none): the slot-major mirrors, [qstride][N] / [hist_cap][N] raw dwords
      {"qcum_t", (void**)&d.qcum_t, sizeof(unsigned) * (size_t)d.qstride, 0, 0},
      {"hist_t", (void**)&d.hist_t, sizeof(unsigned) * (size_t)d.hist_cap, 0, 0},
  };
  // scale starts at 1, last_delta = None (envs/dc_gym.py:81-83)
  {
    std::vector<int> ones(N, 1), none(N, -2);
    if (rec_put(h, R_SCALE, 1, ones.data()) != 0 || rec_put(h, R_LAST_DELTA, 1, none.data()) != 0) {
      sdc_destroy(h);
      return -1;
    }
  }
  *out = h;
  return 0;
}

int sdc_destroy(sdc_handle* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  stage_destroy(h->clone_stage);
  stage_destroy(h->idx_stage);
  stage_destroy(h->plan_stage);
  if (h->plan_rows) (void)hipFree(h->plan_rows);
  if (h->plan_out) (void)hipFree(h->plan_out);
  if (h->plan_fc) (void)hipFree(h->plan_fc);
  if (h->plan_saved) (void)hipFree(h->plan_saved);
  if (h->policy_out) (void)hipFree(h->policy_out);
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
  return 0;
}

int sdc_set_seed(sdc_handle* h, uint64_t seed) {
  if (!h) return fail_msg("sdc_set_seed: null handle");
  h->cfg.seed = seed;
  h->d.seed = seed;
  return 0;
}

int sdc_weather_window_len(const sdc_handle* h) { return h ? h->d.lw : -1; }
int sdc_hist_stride(const sdc_handle* h) { return h ? SDC_HIST_STRIDE : -1; }
int sdc_queue_stride(const sdc_handle* h) { return h ? h->d.qstride : -1; }

int sdc_set_tables(sdc_handle* h, int loc_id, const double* W, const double* C, const double* T, const double* WB,
                   int n) {
  if (refused(sdc_set_tables_refused(call_facts(h), loc_id, W, C, T, WB, n))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  const size_t off = (size_t)loc_id * SDC_TABLE_LEN, bytes = sizeof(double) * SDC_TABLE_LEN;
  HIP_TRY(hipMemcpy(const_cast<double*>(h->d.tabW) + off, W, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(const_cast<double*>(h->d.tabC) + off, C, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(const_cast<double*>(h->d.tabT) + off, T, bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(const_cast<double*>(h->d.tabWB) + off, WB, bytes, hipMemcpyHostToDevice));
  if (invalidate_features(h)) return -1;
  h->tables_set = true;
  return 0;
}

int sdc_set_dc_params(sdc_handle* h, int cfg_id, const sdc_dc_params* p) {
  if (refused(sdc_set_dc_params_refused(call_facts(h), cfg_id, p))) return -2;
  SdcDcDev e;
  if (const char* refused = sdc_derive_dc(*p, e)) return fail_msg(refused);      // (sdc_setup.hpp: reciprocals, rack classes)
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(const_cast<SdcDcDev*>(h->d.dc) + cfg_id, &e, sizeof(e), hipMemcpyHostToDevice));
  h->dc_host[cfg_id] = e;
  h->dc_set[cfg_id] = 1;
  return rebuild_config_tables(h);
}

int sdc_assign_envs(sdc_handle* h, const int32_t* loc_id, const int32_t* cfg_id, const int32_t* day_lo,
                    const int32_t* day_hi) {
  if (refused(sdc_assign_envs_refused(call_facts(h), loc_id, cfg_id, day_lo, day_hi))) return -2;
  const int N = h->cfg.n_envs;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  if (rec_put(h, R_LOC, 1, loc_id) || rec_put(h, R_CFG, 1, cfg_id) || rec_put(h, R_DAY_LO, 1, day_lo) ||
      rec_put(h, R_DAY_HI, 1, day_hi) || invalidate_features(h))
    return -1;
  // the CRAC set-point starts at the config's initial value (make_envs_pyenv.py:124) and is never reset
  if (!h->started) {
    std::vector<double> st(N);
    for (int e = 0; e < N; e++) st[e] = h->dc_host[(size_t)cfg_id[e]].p.init_setpoint;      // (a config not set yet: 0.0)
    if (rec_put(h, R_STPT, 2, st.data())) return -1;
  }
  h->assigned = true;
  h->mirror.set_cfg_ids(cfg_id);
  h->mirror.set_loc_ids(loc_id);
  return rebuild_config_tables(h);
}

int sdc_reset(sdc_handle* h, const uint8_t* mask_host, const sdc_reset_override* ovr, float* obs, float* share_obs,
              void* stream) {
  if (refused(sdc_reset_refused(call_facts(h), mask_host, ovr))) return -2;      // (the overrides' ranges included)
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = h->cfg.n_envs;
  SdcDev d = h->d;
  if (mask_host) {
    HIP_TRY(hipMemcpyAsync(d.reset_mask, mask_host, (size_t)N, hipMemcpyHostToDevice, st));
  } else {
    d.reset_mask = nullptr;
  }
  double* inj_noise = nullptr;
  int* inj_roll = nullptr;
  const bool inject_noise = ovr && ovr->noise;
  if (inject_noise) {
    // the reference's own draws, the arithmetic on the device: day / hour / roll + the year's noise array per env
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&inj_noise), sizeof(double) * (size_t)N * SDC_TABLE_LEN));
    if (hipMalloc(reinterpret_cast<void**>(&inj_roll), sizeof(int) * (size_t)N) != hipSuccess) {
      (void)hipFree(inj_noise);
      return fail_msg("sdc_reset: allocation for the injected roll failed");
    }
    hipError_t e1 = hipMemcpy(inj_noise, ovr->noise, sizeof(double) * (size_t)N * SDC_TABLE_LEN, hipMemcpyHostToDevice);
    hipError_t e2 = hipMemcpy(inj_roll, ovr->roll_days, sizeof(int) * (size_t)N, hipMemcpyHostToDevice);
    hipError_t e3 = hipMemcpy(h->ovr_day, ovr->day, sizeof(int) * (size_t)N, hipMemcpyHostToDevice);
    hipError_t e4 = hipMemcpy(h->ovr_hour, ovr->hour, sizeof(int) * (size_t)N, hipMemcpyHostToDevice);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess) {
      (void)hipFree(inj_noise);
      (void)hipFree(inj_roll);
      return fail_msg("sdc_reset: upload of the injected noise failed");
    }
  } else if (ovr) {
    HIP_TRY(hipMemcpyAsync(h->ovr_day, ovr->day, sizeof(int) * (size_t)N, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->ovr_hour, ovr->hour, sizeof(int) * (size_t)N, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->ovr_ci_min, ovr->ci_min, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->ovr_ci_max, ovr->ci_max, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->ovr_t_min, ovr->t_min, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->ovr_t_max, ovr->t_max, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st));
    const size_t row = sizeof(double) * (size_t)d.lw;
    if (!mask_host) {
      HIP_TRY(hipMemcpyAsync(d.t_win, ovr->t_win, row * N, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d.wb_win, ovr->wb_win, row * N, hipMemcpyHostToDevice, st));
    } else {
      for (int e = 0; e < N; e++) {
        if (!mask_host[e]) continue;
        HIP_TRY(hipMemcpyAsync(d.t_win + (size_t)e * d.lw, ovr->t_win + (size_t)e * d.lw, row, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d.wb_win + (size_t)e * d.lw, ovr->wb_win + (size_t)e * d.lw, row, hipMemcpyHostToDevice, st));
      }
    }
    // the host buffers may be pageable: the copies above must have consumed them before we return
    HIP_TRY(hipStreamSynchronize(st));
  }
  hipLaunchKernelGGL(sdc_reset_kernel, dim3(N), dim3(SDC_WAVE), 0, st, d, inject_noise ? 2 : (ovr ? 1 : 0), h->ovr_day,
                     h->ovr_hour, h->ovr_ci_min, h->ovr_ci_max, h->ovr_t_min, h->ovr_t_max, 0, obs, share_obs, inj_noise,
                     inj_roll);
  launch_features(h, d, st);
  if (inject_noise) {
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(inj_noise);
    (void)hipFree(inj_roll);
    if (es != hipSuccess) return fail("sdc_reset: injected reset", es);
  }
  HIP_TRY(hipGetLastError());
  // the closed loop's copy of the latest observations: a reset without an observation buffer leaves it stale (the next
  // sdc_rollout_actor refuses until a reset / step has delivered observations), and a MASKED reset only wrote the masked
  // envs' rows of `obs` -- the other rows of the caller's buffer are whatever it held, so only those rows are taken over
  if (h->obs_latch && !obs) h->latch_valid = false;
  if (h->obs_latch && obs && mask_host) {
    const size_t row = sizeof(float) * SDC_OBS_OUT;
    for (int e = 0; e < N;) {
      if (!mask_host[e]) { e++; continue; }
      int e1 = e;
      while (e1 < N && mask_host[e1]) e1++;
      HIP_TRY(hipMemcpyAsync(h->obs_latch + (size_t)e * SDC_OBS_OUT, obs + (size_t)e * SDC_OBS_OUT, row * (size_t)(e1 - e),
                             hipMemcpyDeviceToDevice, st));
      e = e1;
    }
  } else if (latch_obs(h, obs, st)) {
    return -1;
  }
  if (mask_host) HIP_TRY(hipStreamSynchronize(st));  // mask staging buffer is reused by the next call
  h->mirror.reset(mask_host);
  h->started = true;
  return 0;
}

int sdc_step(sdc_handle* h, const int32_t* actions, float* obs, float* share_obs, float* rew, uint8_t* done,
             float* info, float* final_obs, void* stream) {
  if (refused(sdc_step_refused(stepping_facts(h), actions, obs, rew, done, info))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = h->cfg.n_envs;
  const bool timed = h->prof > 0 && (h->prof_tick++ % h->prof) == 0 && h->prof_used < PROF_SLOTS;
  SdcDev d = h->d;
  if (timed) {
    d.prof_ts = h->prof_buf + (size_t)h->prof_used * 3 * N * 2;
    h->prof_has_reset[h->prof_used] = 0;
  }
  d.step_no = h->step_no;
  h->step_no = next_step_no(h->step_no, 1);
  const SdcStepPath path = sdc_single_step_path(step_facts(h, actions != nullptr, obs, share_obs, info, final_obs, nullptr, timed));
  launch_step(h, d, path, h->mirror.rel_hint(), actions, obs, share_obs, done, info, final_obs, rew, st);
  if (h->cfg.debug_flags & SDC_DEBUG_VERIFY) hipLaunchKernelGGL(sdc_reward_verify_kernel, dim3(N), dim3(SDC_BLOCK), 0, st, d, info);
  return finish_launch(h, d, 1, obs, share_obs, st, timed, true);
}

int sdc_rollout(sdc_handle* h, int n_steps, const int32_t* actions, float* obs, float* share_obs, float* rew,
                uint8_t* done, float* info, float* final_obs, int32_t* actions_out, void* stream) {
  if (refused(sdc_rollout_refused(stepping_facts(h), n_steps, actions, obs, rew, done))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = h->cfg.n_envs;
  SdcDev d = h->d;
  d.actions_out = actions_out;
  const SdcRolloutPath rp = sdc_rollout_path(step_facts(h, actions != nullptr, obs, share_obs, info, final_obs, actions_out, false));
  if (rp.per_step) {
    // A batch the lane-per-env kernel serves (sdc_wide.hip), from SDC_WIDE_ROLLOUT_MIN_ENVS envs: n_steps single-step launches of it, the
    // deferred re-centrings running between them as in sdc_step -- faster than one n_steps launch of four envs per wavefront
    // (16 384 envs: 17.7 against 23.4 us per step), the same outputs to the bit.  Its general form likewise: several configs,
    // rule-based policies (a step's policy reads the state the previous launch left), other reward functions.
    for (int k = 0; k < n_steps; k++) {
      d.step_no = h->step_no;
      h->step_no = next_step_no(h->step_no, 1);
      const size_t o = (size_t)k * N;
      d.actions_out = actions_out ? actions_out + o * 3 : nullptr;
      const int rel = h->mirror.rel_hint(), rel_k = rel >= 0 ? rel + k : rel;
      launch_step(h, d, rp.path, rel_k, actions ? actions + o * 3 : nullptr, obs + o * SDC_OBS_OUT, share_obs + o * SDC_SHARE_OBS_DIM,
                  done + o, info + o * SDC_INFO_DIM, final_obs, rew + o * 3, st);
    }
  } else {
    // (a multi-step launch has no spare wavefronts between its steps: it re-centres inline, and requests left by the
    // step before it are dropped -- their results would describe a ring several steps old)
    h->step_no = next_step_no(h->step_no, 0);        // (room for the launch's n_steps stamps below the wrap)
    d.step_no = h->step_no;
    h->step_no = next_step_no(h->step_no, n_steps + 3);
    HIP_TRY(hipMemsetAsync(d.rq_count, 0, sizeof(int) * 4, st));
    launch_rollout(h, d, rp.path, n_steps, actions, obs, share_obs, done, info, final_obs, rew, st);
  }
  const size_t last = (size_t)(n_steps - 1) * N;      // the LAST step's slices
  return finish_launch(h, d, n_steps, obs + last * SDC_OBS_OUT, share_obs ? share_obs + last * SDC_SHARE_OBS_DIM : nullptr, st, false, true);
}

int sdc_set_actor(sdc_handle* h, int slot, const sdc_actor_params* p) {
  if (refused(sdc_set_actor_refused(call_facts(h), slot, p))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  if (!h->actor[0].params) {
    if (nets_alloc(h, h->actor, 3, SDC_ACTOR_N_PARAMS, SDC_ACT_IN, SDC_ACTOR_GRAD_MAX_BLOCKS, sdc_actor_pack_tables()) != 0) return -1;
    if (dev_alloc(h, &h->obs_latch, (size_t)h->cfg.n_envs * SDC_OBS_OUT) != 0) return -1;
    h->latch_valid = false;      // (filled by the next reset / step / rollout)
  }
  // torch's [out][in] rows -> the kernel's k-major layout, four consecutive k per lane (sdc_actor.hpp)
  // (per call, on the heap: 26 KB is too large for the stack, and a function-static buffer would be shared by engines on
  // other host threads -- ctypes releases the GIL during this call)
  std::unique_ptr<SdcActorDev> loop(new SdcActorDev);
  sdc_actor_pack(p, loop.get());
  // ... and the same parameters as sdc_actor_evaluate's kernel reads them (sdc_actor_eval_pack.hpp)
  std::unique_ptr<SdcActorEvalDev> packed(new SdcActorEvalDev);
  sdc_actor_eval_pack(p, packed.get());
  // ... and their transposes as sdc_actor_backward's kernel reads them (sdc_actor_grad_pack.hpp)
  std::unique_ptr<SdcActorGradDev> packed_t(new SdcActorGradDev);
  sdc_actor_grad_pack(p, packed_t.get());
  const void* const packs[SDC_ACTOR_N_PACKS] = {loop.get(), packed.get(), packed_t.get()};
  return net_install(h->actor[slot], p, packs, p->activation, p->use_feature_normalization != 0);
}

int sdc_rollout_actor(sdc_handle* h, int n_steps, int sample, float* obs, float* share_obs, float* rew, uint8_t* done,
                      float* info, float* final_obs, int32_t* actions_out, float* logits_out, void* stream) {
  // the common case only, with the actions coming from the actors instead of the caller
  const SdcStepFacts step = h ? step_facts(h, true, obs, share_obs, info, final_obs, actions_out, false) : SdcStepFacts{};
  if (refused(sdc_rollout_actor_refused(stepping_facts(h), step, n_steps, obs, share_obs, rew, done, info, actions_out))) return -2;
  const SdcActorPath ap = sdc_actor_path(step);
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = h->cfg.n_envs;
  SdcDev d = h->d;
  d.actions_out = nullptr;
  h->step_no = next_step_no(h->step_no, 0);
  d.step_no = h->step_no;
  h->step_no = next_step_no(h->step_no, n_steps + 3);
  HIP_TRY(hipMemsetAsync(d.rq_count, 0, sizeof(int) * 4, st));
  if (!h->actor_lds_set) {     // (a per-device attribute: once per handle, not once per process)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(sdc_rollout_actor_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sdc_rollout_actor_lds_bytes()));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(sdc_rollout_actor_quad_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)sdc_rollout_actor_quad_lds_bytes()));
    h->actor_lds_set = true;
  }
  const bool quad = ap.path == SDC_PATH_QUAD;      // four envs per wavefront (batches above 4096 envs)
  const SdcKernelInfo k = sdc_kernel_of(ap.path, SDC_LAUNCH_ACTOR);
  h->last_step_kernel = k.name;
  hipLaunchKernelGGL(quad ? sdc_rollout_actor_quad_kernel : sdc_rollout_actor_kernel, dim3(sdc_env_blocks(k, N)),
                     dim3(SDC_WAVE * k.waves_per_block), quad ? sdc_rollout_actor_quad_lds_bytes() : sdc_rollout_actor_lds_bytes(), st, d,
                     n_steps, h->mirror.rel_hint(), h->actor[0].pack_as<SdcActorDev>(SDC_ACTOR_PACK_LOOP), h->obs_latch, sample ? 1 : 0, obs, share_obs, done, info, final_obs, rew,
                     actions_out, logits_out, h->obs_latch);
  // (after an auto-reset alone: the next launch starts from the reset observations)
  const size_t last = (size_t)(n_steps - 1) * N;
  return finish_launch(h, d, n_steps, obs + last * SDC_OBS_OUT, share_obs + last * SDC_SHARE_OBS_DIM, st, false, false);
}

int sdc_steps_to_episode_end(const sdc_handle* h) { return h ? h->mirror.steps_to_terminal() : -1; }

const char* sdc_last_step_kernel(const sdc_handle* h) { return h ? h->last_step_kernel : ""; }

int sdc_last_done(const sdc_handle* h, uint8_t* done_host) {
  if (!h) return -1;
  if (h->mirror.n_last_done() > 0 && done_host) std::memcpy(done_host, h->mirror.last_done(), (size_t)h->cfg.n_envs);
  return h->mirror.n_last_done();
}

int sdc_profile_enable(sdc_handle* h, int enable) {
  if (refused(sdc_profile_enable_refused(stepping_facts(h)))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  if (enable > 0 && !h->prof_buf) {
    if (dev_alloc(h, &h->prof_buf, (size_t)PROF_SLOTS * 3 * h->cfg.n_envs * 2) != 0) return -1;
    h->prof_has_reset.assign(PROF_SLOTS, 0);
    HIP_TRY(hipMemset(h->prof_buf, 0, sizeof(unsigned long long) * PROF_SLOTS * 3 * h->cfg.n_envs * 2));
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) == hipSuccess && khz > 0)
      h->wall_clock_khz = khz;
  }
  h->prof = enable > 0 ? enable : 0;
  h->prof_tick = 0;
  return 0;
}

int sdc_profile_read(sdc_handle* h, double* out5, int reset) {
  if (refused(sdc_profile_read_refused(stepping_facts(h), out5))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t N = (size_t)h->cfg.n_envs;
  if (h->prof_used > 0) {
    std::vector<unsigned long long> ts((size_t)h->prof_used * 3 * N * 2);
    HIP_TRY(hipMemcpy(ts.data(), h->prof_buf, ts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int s = 0; s < h->prof_used; s++) {
      for (int k = 0; k < 3; k++) {
        if (k == SDC_PROF_RESET && !h->prof_has_reset[s]) continue;
        const unsigned long long* p = ts.data() + ((size_t)s * 3 + k) * N * 2;
        unsigned long long t0 = ~0ull, t1 = 0ull;
        for (size_t e = 0; e < N; e++) {
          if (p[2 * e] == 0ull) continue;   // this workgroup did not run (ring path: only the queued envs)
          t0 = std::min(t0, p[2 * e]);
          t1 = std::max(t1, p[2 * e + 1]);
        }
        if (t1 > t0) h->acc_ms[k] += (double)(t1 - t0) / h->wall_clock_khz;   // first workgroup in -> last workgroup out
      }
      h->acc_ms[3] += 1;
      h->acc_ms[4] += h->prof_has_reset[s];
    }
    h->prof_used = 0;
    HIP_TRY(hipMemset(h->prof_buf, 0, sizeof(unsigned long long) * PROF_SLOTS * 3 * N * 2));
  }
  for (int i = 0; i < 5; i++) out5[i] = h->acc_ms[i];
  if (reset)
    for (int i = 0; i < 5; i++) h->acc_ms[i] = 0;
  return 0;
}

static const Field* find_field(sdc_handle* h, const char* name) {
  if (!h || !name) return nullptr;
  for (const Field& f : h->fields)
    if (std::strcmp(f.name, name) == 0) return &f;
  return nullptr;
}
// ... as the rules of sdc_get_state / sdc_set_state see it (sdc_refusals.hpp)
static SdcFieldFacts field_facts(const Field* f) { return {f ? f->elem : 0, f && (!f->ptr || *f->ptr)}; }

int sdc_get_state(sdc_handle* h, const char* field, void* host_buf, size_t bytes) {
  const Field* f = find_field(h, field);
  const SdcFieldFacts ff = field_facts(f);
  if (refused(sdc_get_state_refused(call_facts(h), field, host_buf, bytes, f ? &ff : nullptr))) return -2;
  const size_t need = f->elem * (size_t)h->cfg.n_envs;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  if (!f->ptr) return rec_get(h, f->rec_idx, f->rec_dwords, host_buf, f->in_hdr);
  HIP_TRY(hipMemcpy(host_buf, *f->ptr, need, hipMemcpyDeviceToHost));
  if (std::strcmp(field, "hist") == 0) {  // device keys -> fp32 offsets (empty slot -> NaN)
    unsigned* u = static_cast<unsigned*>(host_buf);
    for (size_t i = 0; i < need / 4; i++) u[i] = sdc_key_f32(u[i]);
  }
  return 0;
}

// the queue table's time-major mirror rebuilt from the table (after a host write to it)
__global__ void sdc_qcum_mirror_kernel(SdcDev S) {
  const int t = (int)blockIdx.x, env = (int)(blockIdx.y * blockDim.x + threadIdx.x);
  if (env < S.n_envs) S.qcum_t[(size_t)t * S.n_envs + env] = S.qtab[(size_t)env * S.qstride + t].x;
}

// ... and the history ring's slot-major mirror from the rings
__global__ void sdc_hist_mirror_kernel(SdcDev S) {
  const int slot = (int)blockIdx.x, env = (int)(blockIdx.y * blockDim.x + threadIdx.x);
  if (env < S.n_envs) S.hist_t[(size_t)slot * S.n_envs + env] = S.hist[(size_t)env * SDC_HIST_STRIDE + slot];
}

int sdc_set_state(sdc_handle* h, const char* field, const void* host_buf, size_t bytes) {
  const Field* f = find_field(h, field);
  const SdcFieldFacts ff = field_facts(f);
  if (refused(sdc_set_state_refused(call_facts(h), field, host_buf, bytes, f ? &ff : nullptr))) return -2;
  const size_t need = f->elem * (size_t)h->cfg.n_envs;
  const bool is_cfg = std::strcmp(field, "cfg_id") == 0, is_record = std::strcmp(field, "record") == 0;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  if (!f->ptr) {
    if (rec_put(h, f->rec_idx, f->rec_dwords, host_buf, f->in_hdr)) return -1;
    if (std::strcmp(field, "hist_len") == 0 || std::strcmp(field, "hist_pos") == 0) {
      if (std::strcmp(field, "hist_len") == 0 && rec_put(h, H_N, 1, host_buf, 1)) return -1;
      if (invalidate_trackers(h)) return -1;
    }
  } else if (std::strcmp(field, "hist") == 0) {  // fp32 offsets -> device keys (NaN -> empty slot)
    if (invalidate_trackers(h)) return -1;
    std::vector<unsigned> k(need / 4);
    const unsigned* u = static_cast<const unsigned*>(host_buf);
    for (size_t i = 0; i < k.size(); i++) k[i] = ((u[i] & 0x7FFFFFFFu) > 0x7F800000u) ? 0xFFFFFFFFu : sdc_f32_key(u[i]);
    HIP_TRY(hipMemcpy(*f->ptr, k.data(), need, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(*f->ptr, host_buf, need, hipMemcpyHostToDevice));
  }
  const int* ids = static_cast<const int*>(host_buf);      // (cfg_id, loc_id: [N]; record: the fields of [N][SDC_REC_DWORDS])
  if (h->cfg.n_dc_configs > 1) {             // the envs' own copies of their configs' scalars follow the assignment
    if (is_cfg || is_record) {
      if (is_cfg) h->mirror.set_cfg_ids(ids);
      else h->mirror.set_cfg_ids(ids + R_CFG, SDC_REC_DWORDS);
      if (rebuild_config_tables(h)) return -1;
    }
  }
  if (std::strcmp(field, "loc_id") == 0) h->mirror.set_loc_ids(ids);
  else if (is_record) h->mirror.set_loc_ids(ids + R_LOC, SDC_REC_DWORDS);
  if (h->d.qcum_t && std::strcmp(field, "qtab") == 0) {
    hipLaunchKernelGGL(sdc_qcum_mirror_kernel, dim3(h->d.qstride, (h->cfg.n_envs + 255) / 256), dim3(256), 0, 0, h->d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  if (h->d.hist_t && std::strcmp(field, "hist") == 0) {
    hipLaunchKernelGGL(sdc_hist_mirror_kernel, dim3(h->d.hist_cap, (h->cfg.n_envs + 255) / 256), dim3(256), 0, 0, h->d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  h->latch_valid = false;                  // (closed loop: the library's copy of the latest observations describes the state before this write)
  h->mirror.mark_kill_all();               // (a mark row holds only what steps change: whatever was written, it may not be that)
  if (invalidate_features(h)) return -1;   // whatever was written, the precomputed observation rows may no longer match it
  // Deferred window re-centrings in flight belong to the state that has just been overwritten: a restored header may
  // carry request stamps (H_PEND) that the NEXT step would find "two steps old" again and take a swept window over --
  // one that already contains the restored step's own insertion, which the take-over would then replay a second time.
  // Moving the launch counter past every stamp (3 steps: requests are served at +1 and taken over at +2) makes all of
  // them stale, in the headers and in the request / result sets alike; the windows concerned are re-requested.
  h->step_no = next_step_no(h->step_no, 3);
  HIP_TRY(hipMemset(h->d.rq_count, 0, sizeof(int) * 4));
  if (std::strcmp(field, "t_rel") == 0 || std::strcmp(field, "record") == 0) {
    std::vector<int> tr(h->cfg.n_envs);
    if (rec_get(h, R_TREL, 1, tr.data())) return -1;
    h->mirror.reload_t_rel(tr.data());
  }
  return 0;
}

// Env dst[k] becomes a copy of env src[k], on the device and ordered on `stream` like a step (sdc_clone.hip).  What is copied and
// what is not, and why the deferred re-centring stamps are cleared rather than the launch counter moved: include/sustaindc_hip.h.
int sdc_clone_envs(sdc_handle* h, const int32_t* src, const int32_t* dst, int n, float* obs, float* share_obs, void* stream) {
  std::vector<int> src_of;      // dst -> its src
  if (refused(sdc_clone_envs_refused(call_facts(h), src, dst, n, src_of))) return -2;      // (every refusal before anything reaches the device)
  const int N = h->cfg.n_envs;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const SdcDev& d = h->d;
  SdcClonePlan P;
  std::memset(&P, 0, sizeof(P));
  P.n = n;
  P.n_envs = N;
  const auto add = [&P](void* base, size_t pitch) { return seg_add(P, SEG_DEMOTE, base, pitch); };
  bool fits = add(d.rec, sizeof(unsigned) * SDC_REC_DWORDS);
  P.hdr_wide = P.n_wide;      // (the next wide segment, if the header becomes one)
  fits = fits && add(d.hdr, sizeof(unsigned) * SDC_HDR_DWORDS) && P.n_wide > P.hdr_wide &&
              add(d.hist, sizeof(unsigned) * SDC_HIST_STRIDE) && add(d.qwin, sizeof(unsigned) * 4 * SDC_WIN) &&
              add(d.qtab, sizeof(uint2) * (size_t)d.qstride) && add(d.t_win, sizeof(double) * (size_t)d.lw) &&
              add(d.wb_win, sizeof(double) * (size_t)d.lw);
  if (d.prm_env) fits = fits && add(const_cast<double*>(d.prm_env), sizeof(double) * 32);
  if (h->obs_latch) fits = fits && add(h->obs_latch, sizeof(float) * SDC_OBS_OUT);
  if (obs) fits = fits && add(obs, sizeof(float) * SDC_OBS_OUT);
  if (share_obs) fits = fits && add(share_obs, sizeof(float) * SDC_SHARE_OBS_DIM);
  if (!fits) return fail_msg("sdc_clone_envs: internal: the copy plan's segment table is too small");
  constexpr int per_block = SDC_CLONE_BLOCK * SDC_CLONE_UNROLL;
  P.bpp = std::max(1, (int)((P.wide_units + per_block - 1) / per_block));
  P.blocks_a = n * P.bpp;
  if (d.feat) {
    P.feat = d.feat;
    P.feat_rows = d.episode_steps + 1;
    P.feat_pair_groups = (n + SDC_CLONE_BLOCK / 8 - 1) / (SDC_CLONE_BLOCK / 8);
    P.blocks_b = P.feat_pair_groups * ((P.feat_rows + SDC_CLONE_FEAT_ROWS - 1) / SDC_CLONE_FEAT_ROWS);
  }
  if (d.qcum_t) {     // (the ring's mirror, where there is one, lies behind the queue table's in the same [row][N] array)
    P.mirror = d.qcum_t;
    P.mirror_rows = d.qstride + (d.hist_t ? d.hist_cap : 0);
    P.mirror_pair_groups = (n + SDC_CLONE_BLOCK - 1) / SDC_CLONE_BLOCK;
  }
  void* pin_slot = nullptr;
  if (stage_acquire(h, h->clone_stage, &pin_slot)) return -1;
  int2* pin = static_cast<int2*>(pin_slot);
  // the pairs sorted by dst: range C's lanes then write consecutive mirror dwords for a contiguous dst range
  int m = 0;
  for (int e = 0; e < N; e++)
    if (src_of[(size_t)e] >= 0) pin[m++] = make_int2(src_of[(size_t)e], e);
  if (stage_commit(h, h->clone_stage, (size_t)n, st, [&P, st](const void* pairs_dev) {
        P.pairs = static_cast<const int2*>(pairs_dev);
        return sdc_clone_launch(P, st);
      }))
    return -1;

  h->mirror.copy_envs(src, dst, n);
  refresh_racks_max(h);
  return 0;
}

// ---- snapshots (sdc_snapshot.hip) ----------------------------------------------------------------------------------------------
// The row layout (sdc_snapshot.hpp) and the segment table of both directions, from this engine's arrays: the wide segments in unit
// order (record, header first), the narrow ones behind them (the caller's obs first), then the feature rows.  Which array is wide
// follows from its pitch alone (every engine array is a hipMalloc allocation, 256-byte aligned; the caller's obs / share_obs rows are
// never wide) and every pitch from episode_steps, so every engine of the same state layout and episode length lays a row out the same
// way.  -> false if a table is too small or a segment is not where the kernels expect it
static bool snap_plan(const sdc_handle* h, SdcSnapPlan& P, size_t& row_bytes, float* obs, float* share_obs) {
  const SdcDev& d = h->d;
  std::memset(&P, 0, sizeof(P));
  P.n_envs = h->cfg.n_envs;
  bool fits = true;
  const auto add = [&P, &fits](void* base, size_t pitch) { fits = seg_add(P, SEG_BY_PITCH, base, pitch) && fits; };
  add(d.rec, sizeof(unsigned) * SDC_REC_DWORDS);                 // wide segment SDC_SNAP_SEG_REC
  add(d.hdr, sizeof(unsigned) * SDC_HDR_DWORDS);                 // wide segment SDC_SNAP_SEG_HDR
  add(d.qwin, sizeof(unsigned) * 4 * SDC_WIN);
  const unsigned q_first = P.wide_units;      // (wide: qstride % 64 == 0 below)
  add(d.qtab, sizeof(uint2) * (size_t)d.qstride);
  add(obs, sizeof(float) * SDC_OBS_OUT);                         // narrow segment SDC_SNAP_SEG_OBS
  add(share_obs, sizeof(float) * SDC_SHARE_OBS_DIM);
  add(d.t_win, sizeof(double) * (size_t)d.lw);
  add(d.wb_win, sizeof(double) * (size_t)d.lw);
  const unsigned h_first = P.wide_units;
  add(d.hist, sizeof(unsigned) * SDC_HIST_STRIDE);
  static_assert(sizeof(unsigned) * SDC_REC_DWORDS % 16 == 0 && sizeof(unsigned) * SDC_HDR_DWORDS % 16 == 0 &&
                sizeof(float) * SDC_OBS_OUT % 16 != 0 && sizeof(float) * SDC_SHARE_OBS_DIM % 16 != 0,
                "record and header wide, the observation rows narrow: the segment indices the kernels name");
  P.qtab_off = 16u * q_first;      // (wide units: 16-byte aligned in the row, as range C's loads need)
  P.hist_off = 16u * h_first;
  P.feat_off = (16u * P.wide_units + 4u * P.narrow_units + 15u) / 16u * 16u;
  size_t bytes = P.feat_off;
  if (d.feat) {
    P.feat = d.feat;
    P.feat_rows = d.episode_steps + 1;
    bytes += sizeof(float) * SDC_FEAT_ROW * (size_t)P.feat_rows;
  }
  row_bytes = (bytes + 255) / 256 * 256;
  P.row_bytes = (unsigned)row_bytes;
  return fits && P.n_wide > SDC_SNAP_SEG_HDR && P.n_narrow > SDC_SNAP_SEG_OBS && d.qstride % 64 == 0 &&
         d.hist_cap <= SDC_HIST_STRIDE;
}

// the grid of ranges A and B for n envs (C and D: the restore's)
static void snap_grid(SdcSnapPlan& P, const int n) {
  constexpr int per_block = SDC_SNAP_BLOCK * SDC_SNAP_UNROLL;
  P.n = n;
  P.bpe = std::max(1, (int)((P.wide_units + per_block - 1) / per_block));
  P.blocks_a = n * P.bpe;
  if (P.feat) {
    P.feat_groups = (n + SDC_SNAP_BLOCK / 8 - 1) / (SDC_SNAP_BLOCK / 8);
    P.blocks_b = P.feat_groups * ((P.feat_rows + SDC_SNAP_FEAT_ROWS - 1) / SDC_SNAP_FEAT_ROWS);
  }
}

// the launch's {env, row, cfg_id, loc_id} through the handle's idx_stage, and the launch
static int snap_launch(sdc_handle* h, SdcSnapPlan& P, const bool save, const std::vector<int4>& ix, hipStream_t st) {
  return stage_send(h, h->idx_stage, ix.data(), ix.size(), st, [&P, save, st](const void* idx_dev) {
    P.idx = static_cast<const int4*>(idx_dev);
    return sdc_snapshot_launch(P, save, st);
  });
}

size_t sdc_snapshot_row_bytes(const sdc_handle* h) {
  if (!h) return 0;
  SdcSnapPlan P;
  size_t bytes = 0;
  (void)snap_plan(h, P, bytes, nullptr, nullptr);
  return bytes;
}

// Env envs[k] -> snapshot row k, ordered on `stream` like a step, read-only on the engine (sdc_snapshot.hip).  What a row holds and
// what the manifest records: include/sustaindc_hip.h.
int sdc_snapshot_envs(sdc_handle* h, const int32_t* envs, int n, void* rows, int32_t* manifest, const float* obs,
                      const float* share_obs, void* stream) {
  if (refused(sdc_snapshot_envs_refused(call_facts(h), envs, n, rows, manifest, obs, share_obs))) return -2;
  SdcSnapPlan P;
  size_t row_bytes = 0;
  if (!snap_plan(h, P, row_bytes, const_cast<float*>(obs), const_cast<float*>(share_obs)))
    return fail_msg("sdc_snapshot_envs: obs / share_obs rows not dword-aligned, or a layout the snapshot plan does not know");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const SdcHostMirror& mir = h->mirror;
  std::vector<int4> ix((size_t)n);
  for (int k = 0; k < n; k++) {
    const int e = envs[k];
    const int cfg = mir.cfg(e), loc = mir.loc(e);
    ix[(size_t)k] = make_int4(e, k, cfg, loc);
    int32_t* m = manifest + (size_t)k * SDC_SNAPSHOT_MANIFEST;
    m[SDC_SNAP_LAYOUT] = (int32_t)state_layout_hash();
    m[SDC_SNAP_EPISODE_STEPS] = h->cfg.episode_steps;
    m[SDC_SNAP_HIST_CAP] = h->cfg.hist_cap;
    m[SDC_SNAP_QUEUE_STRIDE] = h->d.qstride;
    m[SDC_SNAP_WINDOW_LEN] = h->d.lw;
    m[SDC_SNAP_T_REL] = mir.t_rel(e);
    m[SDC_SNAP_FEAT_OK] = mir.feat(e) ? 1 : 0;
    m[SDC_SNAP_CFG_ID] = cfg;
    m[SDC_SNAP_LOC_ID] = loc;
  }
  P.rows = static_cast<unsigned char*>(rows);
  snap_grid(P, n);
  return snap_launch(h, P, true, ix, st);
}

// Env envs[k] becomes snapshot row rows_idx[k] (sdc_snapshot.hip), ordered on `stream` like a step; the host's mirror follows the
// manifest, so a restore that leaves the batch in lock-step keeps rel_hint and the specialised kernels
int sdc_restore_envs(sdc_handle* h, const int32_t* rows_idx, const int32_t* envs, int n, const void* rows, int n_rows,
                     const int32_t* manifest, float* obs, float* share_obs, void* stream) {
  std::vector<int> row_of;      // dst -> its row
  if (refused(sdc_restore_envs_refused(call_facts(h), rows_idx, envs, n, rows, n_rows, manifest, obs, share_obs, row_of))) return -2;
  const int N = h->cfg.n_envs;
  SdcSnapPlan P;
  size_t row_bytes = 0;
  if (!snap_plan(h, P, row_bytes, obs, share_obs))
    return fail_msg("sdc_restore_envs: obs / share_obs rows not dword-aligned, or a layout the snapshot plan does not know");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const SdcDev& d = h->d;
  P.rows = static_cast<unsigned char*>(const_cast<void*>(rows));
  P.obs_latch = h->obs_latch;
  snap_grid(P, n);
  if (d.qcum_t) {      // C: the mirrors, in tiles of 64 dst envs (qstride is a multiple of 64: whole tiles of 16 queue-table slots)
    P.qcum_t = d.qcum_t;
    P.qstride = d.qstride;
    P.q_tiles = d.qstride / (SDC_SNAP_TILE_BYTES / 8);
    if (d.hist_t) {    // (the row holds SDC_HIST_STRIDE >= hist_cap ring slots: the last tile's reads stay inside it)
      P.hist_t = d.hist_t;
      P.hist_cap = d.hist_cap;
      P.h_tiles = (d.hist_cap + SDC_SNAP_TILE_BYTES / 4 - 1) / (SDC_SNAP_TILE_BYTES / 4);
    }
    P.tile_groups = (n + SDC_SNAP_TILE_ENVS - 1) / SDC_SNAP_TILE_ENVS;
    P.blocks_c = P.tile_groups * (P.q_tiles + P.h_tiles);
  }
  if (d.prm_env && h->prm_cfg_dev) {      // D: the per-env config scalars (several configs)
    P.prm_env = const_cast<double*>(d.prm_env);
    P.prm_cfg = h->prm_cfg_dev;
    P.blocks_d = (n + SDC_SNAP_BLOCK / 16 - 1) / (SDC_SNAP_BLOCK / 16);
  }
  // sorted by dst: range C's wavefronts then write consecutive mirror dwords for a contiguous dst range
  std::vector<int4> ix;
  ix.reserve((size_t)n);
  for (int e = 0; e < N; e++)
    if (row_of[(size_t)e] >= 0) {
      const int32_t* m = manifest + (size_t)row_of[(size_t)e] * SDC_SNAPSHOT_MANIFEST;
      ix.push_back(make_int4(e, row_of[(size_t)e], m[SDC_SNAP_CFG_ID], m[SDC_SNAP_LOC_ID]));
    }
  if (snap_launch(h, P, false, ix, st)) return -1;

  // the host's copy follows the manifest
  std::vector<SdcEnvFacts> facts;
  facts.reserve(ix.size());
  for (const int4& x : ix) {
    const int32_t* m = manifest + (size_t)x.y * SDC_SNAPSHOT_MANIFEST;
    facts.push_back({x.x, m[SDC_SNAP_T_REL], m[SDC_SNAP_FEAT_OK] != 0, m[SDC_SNAP_CFG_ID], m[SDC_SNAP_LOC_ID]});
  }
  h->mirror.replace_envs(facts.data(), facts.size());
  refresh_racks_max(h);
  return 0;
}

// ---- marks (sdc_mark.hip) --------------------------------------------------------------------------------------------------------
// What a mark row holds and why that is enough: include/sustaindc_hip.h; the row layout: sdc_mark.hpp.
size_t sdc_mark_row_bytes(int max_steps) {
  if (max_steps < 1 || max_steps > SDC_MARK_MAX_STEPS) return 0;
  return ((size_t)SDC_MARK_FIXED_BYTES + 12u * (size_t)max_steps + 255u) / 256u * 256u;
}

// the part of the plan both directions share.  -> false: observation rows that are not dword-aligned
static bool mark_plan(const sdc_handle* h, SdcMarkPlan& P, const int n, const int max_steps, const void* rows, const float* obs,
                      const float* share_obs) {
  const SdcDev& d = h->d;
  std::memset(&P, 0, sizeof(P));
  P.n = n;
  P.n_envs = h->cfg.n_envs;
  P.max_steps = max_steps;
  P.hist_cap = d.hist_cap;
  P.qstride = d.qstride;
  P.rows = static_cast<unsigned char*>(const_cast<void*>(rows));
  P.row_bytes = (unsigned)sdc_mark_row_bytes(max_steps);
  P.rec = d.rec;
  P.hdr = d.hdr;
  P.qwin = d.qwin;
  P.hist = d.hist;
  P.qtab = reinterpret_cast<unsigned*>(d.qtab);
  P.obs = const_cast<float*>(obs);
  P.share_obs = const_cast<float*>(share_obs);
  P.blocks_a = (n + SDC_MARK_ENVS_PER_BLOCK - 1) / SDC_MARK_ENVS_PER_BLOCK;
  return ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(share_obs)) & 3u) == 0 && d.hist_cap >= 1 &&
         d.hist_cap <= SDC_HIST_STRIDE && d.qstride >= 1;
}

// the launch's {env, row} pairs (sorted by env: range M's lanes are then consecutive envs) through the handle's idx_stage, and the
// launch; `whole` (envs == NULL): nothing to stage.  row_of: env -> its row, -1 for the others
static int mark_launch(sdc_handle* h, SdcMarkPlan& P, const bool save, const std::vector<int>& row_of, const bool whole,
                       hipStream_t st) {
  if (whole) {
    HIP_TRY(sdc_mark_launch(P, save, st));
    return 0;
  }
  std::vector<int4> ix;
  ix.reserve((size_t)P.n);
  for (int e = 0; e < P.n_envs; e++)
    if (row_of[(size_t)e] >= 0) ix.push_back(make_int4(e, row_of[(size_t)e], 0, 0));
  return stage_send(h, h->idx_stage, ix.data(), ix.size(), st, [&P, save, st](const void* idx_dev) {
    P.idx = static_cast<const int4*>(idx_dev);
    return sdc_mark_launch(P, save, st);
  });
}

// What the next max_steps steps can change in env envs[k] -> mark row k, ordered on `stream` like a step, read-only on the engine.  The
// env's earlier mark is dead from here on.
int sdc_mark_envs(sdc_handle* h, const int32_t* envs, int n, int max_steps, void* rows, int32_t* manifest, const float* obs,
                  const float* share_obs, void* stream) {
  std::vector<int> row_of;
  if (refused(sdc_mark_envs_refused(call_facts(h), envs, n, max_steps, rows, manifest, obs, share_obs, row_of))) return -2;
  SdcMarkPlan P;
  if (!mark_plan(h, P, n, max_steps, rows, obs, share_obs)) return fail_msg("sdc_mark_envs: obs / share_obs rows not dword-aligned");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mark_launch(h, P, true, row_of, envs == nullptr, st)) return -1;
  // the bookkeeping behind the launch: the device is already at work while the host fills the manifest
  if (!h->mark_engine_id) {
    static std::atomic<int> ids{0};
    h->mark_engine_id = ++ids;
  }
  const int serial = h->mirror.mark(envs, n);
  const int32_t layout = (int32_t)state_layout_hash();
  for (int k = 0; k < n; k++) {
    const int e = envs ? envs[k] : k;
    int32_t* m = manifest + (size_t)k * SDC_MARK_MANIFEST;
    m[SDC_MARK_M_LAYOUT] = layout;
    m[SDC_MARK_M_ENGINE] = h->mark_engine_id;
    m[SDC_MARK_M_STEPS] = max_steps;
    m[SDC_MARK_M_ENV] = e;
    m[SDC_MARK_M_SERIAL] = serial;
    m[SDC_MARK_M_T_REL] = h->mirror.t_rel(e);
    m[SDC_MARK_M_HIST_CAP] = h->cfg.hist_cap;
  }
  return 0;
}

// Mark row k -> env envs[k], the slot it was taken from; the host's mirror follows the manifest, so a whole-batch rewind of a lock-step
// batch keeps rel_hint and the specialised kernels.  The mark stays alive: a rewind may be repeated.
int sdc_rewind_envs(sdc_handle* h, const int32_t* envs, int n, const void* rows, const int32_t* manifest, float* obs, float* share_obs,
                    void* stream) {
  // every refusal before anything reaches the device, from the host's mirror; a mark that has been overrun dies whatever the call answers
  std::vector<int> row_of, overrun;
  const int rc = refused(sdc_rewind_envs_refused(call_facts(h), envs, n, rows, manifest, obs, share_obs, row_of, overrun));
  for (const int e : overrun) h->mirror.mark_kill(e);
  if (rc) return rc;
  SdcHostMirror& mir = h->mirror;
  const int max_steps = manifest[SDC_MARK_M_STEPS];
  SdcMarkPlan P;
  if (!mark_plan(h, P, n, max_steps, rows, obs, share_obs)) return fail_msg("sdc_rewind_envs: obs / share_obs rows not dword-aligned");
  const SdcDev& d = h->d;
  P.obs_latch = h->obs_latch;
  if (d.qcum_t) {      // M: the mirrors' rows of the rewound slots
    P.qcum_t = d.qcum_t;
    P.hist_t = d.hist_t;
    P.m_chunks = (max_steps + SDC_MARK_MIRROR_J - 1) / SDC_MARK_MIRROR_J;
    P.blocks_m = (n + SDC_MARK_BLOCK - 1) / SDC_MARK_BLOCK * P.m_chunks;
  }
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mark_launch(h, P, false, row_of, envs == nullptr, st)) return -1;
  // the host's copy follows the manifest: the episode step alone (feature rows, config and trace set are the episode's: unchanged)
  mir.rewind(envs, n, manifest + SDC_MARK_M_T_REL, SDC_MARK_MANIFEST);
  return 0;
}

// ---- plan (sdc_plan.hip) ---------------------------------------------------------------------------------------------------------
// The contract and the arithmetic: include/sustaindc_hip.h; the output block and the kernels' plans: sdc_plan.hpp.

// a buffer of the handle's that only grows (hipFree waits for whatever may still use the old one)
static int plan_grow(unsigned char** buf, size_t* have, const size_t need) {
  if (*have >= need) return 0;
  if (*buf) {
    HIP_TRY(hipFree(*buf));
    *buf = nullptr;
    *have = 0;
  }
  void* q = nullptr;
  HIP_TRY(hipMalloc(&q, need));
  *buf = static_cast<unsigned char*>(q);
  *have = need;
  return 0;
}

// a kernel launch's error -> the call's return code, with the message set
static int launched(const char* kernel, const hipError_t e) { return e != hipSuccess ? fail(kernel, e) : 0; }

// ---- plan forecast (sdc_forecast.hip) --------------------------------------------------------------------------------------------------
// Host state of the handle; plan_session overlays it.  The contract: include/sustaindc_hip.h.

// bit c: channel c of the handle's forecast is not PERFECT (0: the plan calls launch what they launch without a forecast)
static unsigned forecast_channels(const sdc_handle* h) {
  unsigned m = 0;
  for (int c = 0; c < SDC_FC_CHANNELS; c++)
    if (h->plan_forecast.mode[c] != SDC_FORECAST_PERFECT) m |= 1u << c;
  return m;
}
// the fill kernel's plan for n_entries entries into fc, with the handle's modes or -- truth -- every channel PERFECT
static SdcForecastFill forecast_fill_plan(const sdc_handle* h, const int n_entries, const bool truth, double* fc) {
  const sdc_plan_forecast& f = h->plan_forecast;
  SdcForecastFill F;
  std::memset(&F, 0, sizeof(F));
  F.n_envs = h->cfg.n_envs;
  F.n_entries = n_entries;
  F.table_len = h->d.table_len;
  F.lw = h->d.lw;
  if (!truth) {
    F.mode_w = f.mode[SDC_FC_W];
    F.mode_c = f.mode[SDC_FC_C];
    F.mode_t = f.mode[SDC_FC_T];
    F.mode_wb = f.mode[SDC_FC_WB];
    F.values = f.values;
  }
  F.rec = h->d.rec;
  F.tabW = h->d.tabW;
  F.tabC = h->d.tabC;
  F.t_win = h->d.t_win;
  F.wb_win = h->d.wb_win;
  F.fc = fc;
  return F;
}

int sdc_set_plan_forecast(sdc_handle* h, const sdc_plan_forecast* fc) {
  sdc_plan_forecast f;
  if (refused(sdc_set_plan_forecast_refused(call_facts(h), fc, f))) return -2;
  h->plan_forecast = f;
  return 0;
}

int sdc_get_plan_forecast(const sdc_handle* h, sdc_plan_forecast* out) {
  if (!h || !out) return fail_msg("sdc_get_plan_forecast: null handle or out");
  *out = h->plan_forecast;
  return 0;
}

int sdc_forecast_traces(sdc_handle* h, int n_entries, int truth, double* out, void* stream) {
  if (refused(sdc_forecast_traces_refused(call_facts(h), n_entries, truth, out))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  return launched("sdc_forecast_fill_kernel",
                  sdc_forecast_fill_launch(forecast_fill_plan(h, n_entries, truth != 0, out), reinterpret_cast<hipStream_t>(stream)));
}

// A plan call's horizon, the layout of the handle's output block for it, and the score kernel's plan but for the candidate's own arrays
struct PlanRun {
  int n_steps, chunk;
  SdcPlanBlock B;
  SdcPlanScore S;
};

// the steps of a call of n_steps that the handle's output block holds at a time, the block's layout for them, and the block grown to it
static int plan_out_block(sdc_handle* h, const int n_steps, int& chunk, SdcPlanBlock& B) {
  const size_t N = (size_t)h->cfg.n_envs;
  chunk = sdc_plan_steps_fit(N, n_steps, SDC_PLAN_SCRATCH_BYTES);
  if (h->cfg.debug_flags & SDC_PLAN_DEBUG_TWO_STEPS) chunk = std::min(chunk, 2);
  B = sdc_plan_block(N, (size_t)chunk);
  return plan_grow(&h->plan_out, &h->plan_out_bytes, B.bytes);
}

// the handle's buffers, before anything is enqueued
static int plan_prepare(sdc_handle* h, const int n_steps, const sdc_plan_objective& obj, PlanRun& R) {
  const size_t N = (size_t)h->cfg.n_envs;
  R.n_steps = n_steps;
  if (plan_grow(&h->plan_rows, &h->plan_rows_bytes, N * sdc_mark_row_bytes(n_steps))) return -1;
  if (plan_out_block(h, n_steps, R.chunk, R.B)) return -1;
  h->plan_manifest.resize(N * SDC_MARK_MANIFEST);
  std::memset(&R.S, 0, sizeof(R.S));
  R.S.n_envs = (int)N;
  R.S.n_cols = obj.n_cols;
  R.S.rew = reinterpret_cast<float*>(h->plan_out + R.B.rew);
  R.S.info = reinterpret_cast<float*>(h->plan_out + R.B.info);
  for (int a = 0; a < 3; a++) R.S.w[a] = obj.reward_weight[a];
  for (int j = 0; j < obj.n_cols; j++) {
    R.S.col[j] = obj.col[j];
    R.S.col_weight[j] = obj.col_weight[j];
  }
  return 0;
}

// n_steps steps rolled out into the handle's output block (layout B, of `chunk` steps) in chunks: rollout(first step, steps, the block's
// obs, share_obs, rew, done, info, final_obs) -> rc, then per_chunk(first step, steps) behind it.  The rollout is an entry point itself --
// sdc_rollout (rollout_of), sdc_rollout_actor (sdc_rollout_actor_stats) -- so the rollouts choose their kernel as that entry point does
// and the host's mirror is kept by the code that keeps it for every other caller.
extern "C++" {
template <class Rollout, class PerChunk>
static int rollout_chunks(sdc_handle* h, const SdcPlanBlock& B, const int n_steps, const int chunk, Rollout&& rollout, PerChunk&& per_chunk) {
  unsigned char* const out = h->plan_out;
  int rc = 0;
  for (int k0 = 0; k0 < n_steps && rc == 0; k0 += chunk) {
    const int steps = std::min(chunk, n_steps - k0);
    rc = rollout(k0, steps, reinterpret_cast<float*>(out + B.obs), reinterpret_cast<float*>(out + B.share_obs),
                 reinterpret_cast<float*>(out + B.rew), out + B.done, reinterpret_cast<float*>(out + B.info),
                 reinterpret_cast<float*>(out + B.final_obs));
    if (rc == 0) rc = per_chunk(k0, steps);
  }
  return rc;
}

// rollout_chunks' rollout for an action sequence: sdc_rollout of actions [n_steps][N][3], or nullptr (built-in policies)
static auto rollout_of(sdc_handle* h, const int32_t* actions, void* stream) {
  return [=](const int k0, const int steps, float* obs, float* share_obs, float* rew, uint8_t* done, float* info, float* final_obs) {
    return sdc_rollout(h, steps, actions ? actions + (size_t)k0 * (size_t)h->cfg.n_envs * 3 : nullptr, obs, share_obs, rew, done, info,
                       final_obs, nullptr, stream);
  };
}
}  // extern "C++"

// What a plan call works with once it has been let through: the run, the device side of its discount table, the discount of the
// handle's terminal term (g[n_steps - 1] * gamma), the caller's obs / share_obs rows (every rewind refreshes them) and stream
struct PlanSession {
  sdc_handle* h;
  PlanRun R;
  const void* g_dev;
  double g_terminal;
  float *obs, *share_obs;
  void* stream;
  hipStream_t st() const { return reinterpret_cast<hipStream_t>(stream); }
};

// the score kernel's plan with the handle's plan terms (sdc_plan_terms.hpp); S is read at the launch
static SdcPlanScoreTerms plan_terms_plan(const PlanSession& P) {
  const sdc_plan_terms& t = P.h->plan_terms;
  SdcPlanScoreTerms T;
  std::memset(&T, 0, sizeof(T));
  T.n_steps = P.R.n_steps;
  T.n_limits = t.n_limits;
  T.n_terminal = t.n_terminal;
  T.g_terminal = P.g_terminal;
  T.cols = sdc_plan_pack_cols(P.R.S.col, P.R.S.n_cols);
  T.limit_cols = sdc_plan_pack_cols(t.limit_col, t.n_limits);
  T.terminal_cols = sdc_plan_pack_cols(t.terminal_col, t.n_terminal);
  for (int j = 0; j < t.n_limits; j++) {
    T.limit_upper |= (t.limit_side[j] > 0 ? 1u : 0u) << j;
    T.limit_bound[j] = t.limit_bound[j];
    T.limit_weight[j] = t.limit_weight[j];
  }
  for (int j = 0; j < t.n_terminal; j++) T.terminal_weight[j] = t.terminal_weight[j];
  return T;
}

// Per candidate: roll out (rollout_chunks), score each chunk, rewind -- from the mark the session has taken into h->plan_rows.  With
// plan terms on the handle the score is sdc_plan_score_terms_kernel's, without it is sdc_plan_score_kernel's; with a plan critic weight
// sdc_critic_terminal_kernel adds the critic's terminal value behind the last chunk's score.
static int plan_candidates(PlanSession& P, const int n_cand, const int32_t* actions, double* returns, double* score) {
  sdc_handle* const h = P.h;
  const size_t N = (size_t)h->cfg.n_envs;
  SdcPlanScore& S = P.R.S;
  S.g = static_cast<const double*>(P.g_dev);
  const bool terms = h->plan_terms.n_limits > 0 || h->plan_terms.n_terminal > 0;
  SdcPlanScoreTerms T = plan_terms_plan(P);
  // the plan critic (sdc_set_plan_critic): behind the score launch of the chunk that holds the horizon's last step, the critic's value
  // of that step's share_obs rows in the block, added into the candidate's score (sdc_critic.hip)
  const double critic_weight = h->plan_critic_weight;
  SdcCriticTerminal V{critic_dev(h), nullptr, nullptr, (int)N, P.g_terminal * critic_weight, nullptr};
  int rc = 0;
  for (int c = 0; c < n_cand && rc == 0; c++) {
    S.returns = returns ? returns + (size_t)c * N * 3 : nullptr;
    S.score = score + (size_t)c * N;
    rc = rollout_chunks(h, P.R.B, P.R.n_steps, P.R.chunk, rollout_of(h, actions + (size_t)c * (size_t)P.R.n_steps * N * 3, P.stream),
                        [&](const int k0, const int steps) {
                          S.first_step = k0;
                          S.steps = steps;
                          if (terms) T.S = S;
                          const int scored = terms ? launched("sdc_plan_score_terms_kernel", sdc_plan_score_terms_launch(T, P.st()))
                                                   : launched("sdc_plan_score_kernel", sdc_plan_score_launch(S, P.st()));
                          if (scored || critic_weight == 0.0 || k0 + steps != P.R.n_steps) return scored;
                          const size_t last = (size_t)(steps - 1) * N;      // the chunk's last step is the horizon's
                          V.rows = reinterpret_cast<const float*>(h->plan_out + P.R.B.share_obs) + last * SDC_SHARE_OBS_DIM;
                          V.done = h->plan_out + P.R.B.done + last;
                          V.score = S.score;
                          h->last_step_kernel = "sdc_critic_terminal_kernel";
                          return launched("sdc_critic_terminal_kernel", sdc_critic_terminal_launch(V, P.st()));
                        });
    if (rc == 0) rc = sdc_rewind_envs(h, nullptr, (int)N, h->plan_rows, h->plan_manifest.data(), P.obs, P.share_obs, P.stream);
  }
  return rc;
}

// The overlay's plan of the handle's forecast (sdc_forecast.hpp) for a plan of n_steps, the handle's two buffers grown to it;
// W.channels == 0: every channel PERFECT, nothing to launch
static int plan_forecast_swap(sdc_handle* h, const int n_steps, SdcForecastSwap& W) {
  const size_t N = (size_t)h->cfg.n_envs;
  std::memset(&W, 0, sizeof(W));
  W.channels = forecast_channels(h);
  if (!W.channels) return 0;
  if (plan_grow(&h->plan_fc, &h->plan_fc_bytes, (size_t)(n_steps + 2) * N * SDC_FC_CHANNELS * sizeof(double))) return -1;
  if (plan_grow(&h->plan_saved, &h->plan_saved_bytes, (size_t)n_steps * N * SDC_FORECAST_SAVED_DWORDS * sizeof(unsigned))) return -1;
  W.n_envs = (int)N;
  W.n_steps = n_steps;
  W.n_rows = h->d.episode_steps + 1;
  W.units = sdc_forecast_units(W.channels);
  W.rec = h->d.rec;
  W.fc = reinterpret_cast<const double*>(h->plan_fc);
  W.feat = h->d.feat;
  W.saved = reinterpret_cast<unsigned*>(h->plan_saved);
  return 0;
}

extern "C++" {
// A plan of P.R.n_steps steps once its buffers are there and its discount table is on the device (P.g_dev, P.g_terminal): the mark of
// the whole batch; the handle's forecast -- behind the mark one fill and one overlay of the rows the rollouts will read, behind the body,
// whatever it returns, the saved bits back; nothing of it with every channel PERFECT --; and body(session) -> rc, which enqueues the
// call's own work.  One mark serves every rollout of the plan: a rewind keeps its mark alive.
template <class Body>
static int plan_marked(PlanSession& P, SdcForecastSwap& W, Body&& body) {
  sdc_handle* const h = P.h;
  const int n_steps = P.R.n_steps;
  int rc = sdc_mark_envs(h, nullptr, h->cfg.n_envs, n_steps, h->plan_rows, h->plan_manifest.data(), P.obs, P.share_obs, P.stream);
  bool overlaid = false;
  if (rc == 0 && W.channels) {
    rc = launched("sdc_forecast_fill_kernel",
                  sdc_forecast_fill_launch(forecast_fill_plan(h, n_steps + 2, false, reinterpret_cast<double*>(h->plan_fc)), P.st()));
    if (rc == 0) rc = launched("sdc_forecast_swap_kernel", sdc_forecast_swap_launch(W, P.st()));
    overlaid = rc == 0;
  }
  if (rc == 0) rc = body(P);
  if (overlaid) {
    W.back = 1;
    const int back = launched("sdc_forecast_swap_kernel", sdc_forecast_swap_launch(W, P.st()));
    if (rc == 0) rc = back;
  }
  return rc;
}

// What the three plan calls do alike once their arguments have passed (plan_refused and their own checks): the handle's buffers, the
// discount table g_k = g_{k-1} * gamma through the plan's stage -- the slot stays in flight until the last kernel that reads it --, and
// behind it the marked plan (plan_marked) with the call's body.
template <class Body>
static int plan_session(sdc_handle* h, const int n_steps, const sdc_plan_objective& obj, float* obs, float* share_obs, void* stream,
                        Body&& body) {
  HIP_TRY(hipSetDevice(h->device));
  PlanSession P{h, {}, nullptr, 0.0, obs, share_obs, stream};
  if (plan_prepare(h, n_steps, obj, P.R)) return -1;
  SdcForecastSwap W;
  if (plan_forecast_swap(h, n_steps, W)) return -1;
  void* pin = nullptr;
  if (stage_acquire(h, h->plan_stage, &pin)) return -1;
  double* const g = static_cast<double*>(pin);
  g[0] = 1.0;
  for (int k = 1; k < n_steps; k++) g[k] = g[k - 1] * obj.gamma;
  P.g_terminal = g[n_steps - 1] * obj.gamma;
  int rc = 0;
  const int staged = stage_commit(h, h->plan_stage, (size_t)n_steps, P.st(), [&](const void* g_dev) {
    P.g_dev = g_dev;
    rc = plan_marked(P, W, body);
    return hipSuccess;
  });
  return rc ? rc : staged;
}
}  // extern "C++"

// Mark, the candidates (plan_candidates), select.  Whatever the entry points underneath would refuse is refused here first.
int sdc_plan(sdc_handle* h, int n_cand, int n_steps, const int32_t* actions, const sdc_plan_objective* objective, double* returns,
             double* score, int32_t* best, int32_t* best_action, float* obs, float* share_obs, void* stream) {
  sdc_plan_objective obj;
  if (refused(sdc_plan_refused(call_facts(h), n_cand, n_steps, actions, objective, score, best, best_action, obs, share_obs, obj))) return -2;
  const SdcPlanSelect Q{h->cfg.n_envs, n_cand, n_steps, score, actions, best, best_action};
  return plan_session(h, n_steps, obj, obs, share_obs, stream, [&](PlanSession& P) {
    const int rc = plan_candidates(P, n_cand, actions, returns, score);
    return rc ? rc : launched("sdc_plan_select_kernel", sdc_plan_select_launch(Q, P.st()));
  });
}

// ---- plan terms (sdc_plan_terms.hip) ---------------------------------------------------------------------------------------------------
// Host state of the handle; plan_candidates reads it.  The contract: include/sustaindc_hip.h.
int sdc_set_plan_terms(sdc_handle* h, const sdc_plan_terms* terms) {
  sdc_plan_terms t;
  if (refused(sdc_set_plan_terms_refused(call_facts(h), terms, t))) return -2;
  h->plan_terms = t;
  return 0;
}

int sdc_get_plan_terms(const sdc_handle* h, sdc_plan_terms* out) {
  if (!h || !out) return fail_msg("sdc_get_plan_terms: null handle or out");
  *out = h->plan_terms;
  return 0;
}

// ---- the critic (sdc_critic.hip) -------------------------------------------------------------------------------------------------------
// The contract: include/sustaindc_hip.h THE CRITIC; the pack and what is refused about the parameters: sdc_critic_pack.hpp.
int sdc_set_critic(sdc_handle* h, const sdc_critic_params* p) {
  if (refused(sdc_set_critic_refused(call_facts(h), p))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  if (!h->critic.params) {
    if (nets_alloc(h, &h->critic, 1, SDC_CRITIC_N_PARAMS, SDC_CRITIC_IN, SDC_CRITIC_GRAD_MAX_BLOCKS, sdc_critic_pack_tables()) != 0) return -1;
    if (dev_alloc(h, &h->value_norm, 1) != 0) return -1;
  }
  std::unique_ptr<SdcCriticDev> packed(new SdcCriticDev);      // (26 KB: on the heap, per call -- see sdc_set_actor)
  sdc_critic_pack(p, packed.get());
  // ... and the transposed weights as sdc_critic_backward's kernel reads them (sdc_critic_grad_pack.hpp)
  std::unique_ptr<SdcCriticGradDev> packed_t(new SdcCriticGradDev);
  sdc_critic_grad_pack(p, packed_t.get());
  const void* const packs[SDC_CRITIC_N_PACKS] = {packed.get(), packed_t.get()};
  if (net_install(h->critic, p, packs, (p->flags >> 1) & 3, (p->flags & 1) != 0) != 0) return -1;
  h->critic_scale = p->scale;
  h->critic_shift = p->shift;
  h->critic_flags = p->flags;
  h->value_norm_installed = false;      // (scale and shift set by hand: no running state)
  return 0;
}

int sdc_critic_values(sdc_handle* h, const float* share_obs, long long n_rows, float* values, void* stream) {
  if (refused(sdc_critic_values_refused(call_facts(h), share_obs, n_rows, values))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  h->last_step_kernel = "sdc_critic_values_kernel";
  return launched("sdc_critic_values_kernel",
                  sdc_critic_values_launch(SdcCriticValues{critic_dev(h), share_obs, n_rows, values}, reinterpret_cast<hipStream_t>(stream)));
}

// ---- the on-policy batch (sdc_onpolicy.hip) ------------------------------------------------------------------------------------------------
// The contract and the arithmetic: include/sustaindc_hip.h THE ON-POLICY BATCH; the kernels' plans: sdc_onpolicy.hpp.
int sdc_gae(sdc_handle* h, int n_steps, const float* rew, int reward_agent, const uint8_t* done, const uint8_t* first_done,
            const float* values, double gamma, double gae_lambda, int use_gae, float* returns, float* advantages, float* masks,
            float* value_preds, double* moments, void* stream) {
  if (refused(sdc_gae_refused(call_facts(h), n_steps, rew, reward_agent, done, values, gamma, gae_lambda, use_gae, returns, advantages,
                              masks, value_preds, moments)))
    return -2;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int N = h->cfg.n_envs;
  if (!h->adv_part && dev_alloc(h, &h->adv_part, (size_t)N * 2, false) != 0) return -1;
  SdcGae P;
  std::memset(&P, 0, sizeof(P));
  P.n_envs = N;
  P.steps = n_steps;
  P.reward_agent = reward_agent;
  P.use_gae = use_gae;
  P.g = (float)gamma;
  P.c = (float)(gamma * gae_lambda);
  P.rew = rew;
  P.done = done;
  P.first_done = first_done;
  P.values = values;
  P.returns = returns;
  P.advantages = advantages;
  P.masks = masks;
  P.value_preds = value_preds;
  P.critic = critic_dev(h);
  P.adv_part = h->adv_part;
  if (const int rc = launched("sdc_gae_kernel", sdc_gae_launch(P, st))) return rc;
  if (!moments) return 0;
  return launched("sdc_adv_moments_kernel",
                  sdc_adv_moments_launch(SdcAdvMoments{N, (double)n_steps * (double)N, h->adv_part, moments}, st));
}

int sdc_action_log_probs(sdc_handle* h, int n_steps, const int32_t* actions, const float* logits, float* log_probs, float* entropy,
                         void* stream) {
  if (refused(sdc_action_log_probs_refused(call_facts(h), n_steps, actions, logits, log_probs, entropy))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  const long long n = (long long)n_steps * h->cfg.n_envs * SDC_N_AGENTS;
  return launched("sdc_action_logp_kernel",
                  sdc_action_logp_launch(SdcActionLogp{n, actions, logits, log_probs, entropy}, reinterpret_cast<hipStream_t>(stream)));
}

// ---- the actors on stored rows, and the PPO terms (sdc_actor_eval.hip) -----------------------------------------------------------------
// The contract and the arithmetic: include/sustaindc_hip.h EVALUATE THE ACTORS ON STORED ROWS; the kernels' plans: sdc_actor_eval.hpp.
int sdc_actor_evaluate(sdc_handle* h, int agent_slot, const float* obs, long long row_stride, long long n_rows, float* logits,
                       long long logits_stride, void* stream) {
  if (refused(sdc_actor_evaluate_refused(call_facts(h), agent_slot, obs, row_stride, n_rows, logits, logits_stride))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  return launched("sdc_actor_eval_kernel",
                  sdc_actor_eval_launch(SdcActorEval{h->actor[agent_slot].pack_as<SdcActorEvalDev>(SDC_ACTOR_PACK_EVAL), obs, row_stride, n_rows, logits, logits_stride},
                                        reinterpret_cast<hipStream_t>(stream)));
}

extern "C++" {
// what sdc_ppo_terms' and sdc_ppo_dlogp's plans share: zeroed, then the elements, the agent, the four inputs and the clip range
template <class Plan>
static Plan ppo_plan(const sdc_handle* h, const int n_steps, const int agent, const float* new_log_probs, const float* old_log_probs,
                     const float* advantages, const float* factor, const double clip_param) {
  Plan P;
  std::memset(&P, 0, sizeof(P));
  P.n = (long long)n_steps * h->cfg.n_envs;
  P.agent = agent;
  P.new_lp = new_log_probs;
  P.old_lp = old_log_probs;
  P.adv = advantages;
  P.factor = factor;
  P.lo = 1.0 - clip_param;
  P.hi = 1.0 + clip_param;
  return P;
}
// both backward calls (sdc_rowmlp_grad.hpp) behind their plan `P`: the partials of the network's kind allocated on first use (`kind`: its
// `count` records), the gradient kernel, then the B partials' fp64 sum into `grads` and, where grad_sq is given, its squares
template <class Plan>
static int net_backward(sdc_handle* h, SdcNet* kind, const int count, const SdcNet& n, Plan& P, const char* grad_kernel,
                        hipError_t (*grad)(const Plan&, int, hipStream_t), const char* reduce_kernel,
                        hipError_t (*reduce)(const SdcRowMlpGradReduce&, hipStream_t), const char* sq_kernel,
                        hipError_t (*sq)(const SdcRowMlpGradSq&, hipStream_t), const long long n_rows, float* grads, double* grad_sq, hipStream_t st) {
  if (!n.grad_part) {
    float* part = nullptr;
    if (dev_alloc(h, &part, (size_t)n.grad_max_blocks * n.n_params, false) != 0) return -1;
    for (int i = 0; i < count; i++) kind[i].grad_part = part;
  }
  P.part = n.grad_part;
  if (const int rc = launched(grad_kernel, grad(P, n.activation, st))) return rc;
  const int n_part = sdc_rowmlp_grad_blocks(n_rows, n.grad_max_blocks);
  if (const int rc = launched(reduce_kernel, reduce(SdcRowMlpGradReduce{n_part, n.grad_part, grads}, st))) return rc;
  if (!grad_sq) return 0;
  return launched(sq_kernel, sq(SdcRowMlpGradSq{grads, grad_sq}, st));
}
}  // extern "C++"

int sdc_ppo_terms(sdc_handle* h, int n_steps, int agent, const float* new_log_probs, const float* old_log_probs, const float* entropy,
                  const float* advantages, const float* factor, double clip_param, float* ratio, float* surr, float* factor_out,
                  double* stats, void* stream) {
  if (refused(sdc_ppo_terms_refused(call_facts(h), n_steps, agent, new_log_probs, old_log_probs, entropy, advantages, factor, clip_param,
                                    ratio, surr, factor_out, stats)))
    return -2;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (stats && !h->ppo_part && dev_alloc(h, &h->ppo_part, (size_t)SDC_PPO_MAX_BLOCKS * SDC_PPO_STATS, false) != 0) return -1;
  SdcPpoTerms P = ppo_plan<SdcPpoTerms>(h, n_steps, agent, new_log_probs, old_log_probs, advantages, factor, clip_param);
  P.entropy = entropy;
  P.ratio = ratio;
  P.surr = surr;
  P.factor_out = factor_out;
  P.part = stats ? h->ppo_part : nullptr;
  if (const int rc = launched("sdc_ppo_terms_kernel", sdc_ppo_terms_launch(P, st))) return rc;
  if (!stats) return 0;
  return launched("sdc_ppo_stats_kernel", sdc_ppo_stats_launch(SdcPpoStats{sdc_ppo_blocks(P.n), (double)P.n, h->ppo_part, stats}, st));
}

// ---- the actors' gradient (sdc_actor_grad.hip) ---------------------------------------------------------------------------------------
// The contract and the arithmetic: include/sustaindc_hip.h THE ACTORS' GRADIENT; the kernels' plans: sdc_actor_grad.hpp.
int sdc_ppo_dlogp(sdc_handle* h, int n_steps, int agent, const float* new_log_probs, const float* old_log_probs, const float* advantages,
                  const float* factor, double clip_param, double scale, float* dlogp, void* stream) {
  if (refused(sdc_ppo_dlogp_refused(call_facts(h), n_steps, agent, new_log_probs, old_log_probs, advantages, factor, clip_param, scale, dlogp)))
    return -2;
  HIP_TRY(hipSetDevice(h->device));
  SdcPpoDlogp P = ppo_plan<SdcPpoDlogp>(h, n_steps, agent, new_log_probs, old_log_probs, advantages, factor, clip_param);
  P.scale = scale;
  P.dlogp = dlogp;
  return launched("sdc_ppo_dlogp_kernel", sdc_ppo_dlogp_launch(P, reinterpret_cast<hipStream_t>(stream)));
}

int sdc_actor_backward(sdc_handle* h, int agent_slot, const float* obs, long long row_stride, long long n_rows, const int32_t* actions,
                       long long action_stride, const float* dlogp, double dent, float* grads, double* grad_sq, void* stream) {
  if (refused(sdc_actor_backward_refused(call_facts(h), agent_slot, obs, row_stride, n_rows, actions, action_stride, dlogp, dent, grads, grad_sq)))
    return -2;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const SdcNet& n = h->actor[agent_slot];
  SdcActorGrad P;
  std::memset(&P, 0, sizeof(P));
  P.actor = n.pack_as<SdcActorEvalDev>(SDC_ACTOR_PACK_EVAL);
  P.actor_t = n.pack_as<SdcActorGradDev>(SDC_ACTOR_PACK_GRAD);
  P.obs = obs;
  P.row_stride = row_stride;
  P.n_rows = n_rows;
  P.actions = actions;
  P.action_stride = action_stride;
  P.dlogp = dlogp;
  P.dent = dent;
  return net_backward(h, h->actor, 3, n, P, "sdc_actor_grad_kernel", sdc_actor_grad_launch, "sdc_actor_grad_reduce_kernel",
                      sdc_actor_grad_reduce_launch, "sdc_actor_grad_sq_kernel", sdc_actor_grad_sq_launch, n_rows, grads, grad_sq, st);
}

// ---- the critic's gradient (sdc_critic_grad.hip) -------------------------------------------------------------------------------------
// The contract and the arithmetic: include/sustaindc_hip.h THE CRITIC'S GRADIENT; the kernels' plans: sdc_critic_grad.hpp.
int sdc_critic_evaluate(sdc_handle* h, const float* share_obs, long long n_rows, float* raw_values, void* stream) {
  if (refused(sdc_critic_evaluate_refused(call_facts(h), share_obs, n_rows, raw_values))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  return launched("sdc_critic_raw_kernel",
                  sdc_critic_raw_launch(SdcCriticRaw{critic_dev(h), share_obs, n_rows, raw_values}, reinterpret_cast<hipStream_t>(stream)));
}

// sdc_value_loss and sdc_value_loss_normed behind their rule: the plan but for the targets' scale and shift (the caller's, or read from
// the ValueNorm `block` on the device), stage 1's partial statistics allocated on first use, and stage 2
static int value_loss(sdc_handle* h, const long long n, const float* raw_values, const float* value_preds, const float* returns,
                      const double target_scale, const double target_shift, const SdcValueNormDev* block, const double clip_param,
                      const double huber_delta, const int flags, const double coef, float* loss, float* dvalue, double* stats, void* stream) {
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (stats && !h->value_loss_part && dev_alloc(h, &h->value_loss_part, (size_t)SDC_PPO_MAX_BLOCKS * SDC_PPO_STATS, false) != 0) return -1;
  SdcValueLoss P;
  std::memset(&P, 0, sizeof(P));
  P.n = n;
  P.raw = raw_values;
  P.vp = value_preds;
  P.ret = returns;
  P.scale = target_scale;
  P.shift = target_shift;
  P.clip = clip_param;
  P.delta = (flags & SDC_VALUE_LOSS_HUBER) ? huber_delta : 0.0;
  P.coef = coef;
  P.flags = flags;
  P.loss = loss;
  P.dvalue = dvalue;
  P.part = stats ? h->value_loss_part : nullptr;
  if (const int rc = block ? launched("sdc_value_loss_normed_kernel", sdc_value_loss_normed_launch(P, block, st))
                           : launched("sdc_value_loss_kernel", sdc_value_loss_launch(P, st)))
    return rc;
  if (!stats) return 0;
  // (stage 2 is sdc_ppo_terms' own: the same seven folds over the partials)
  return launched("sdc_ppo_stats_kernel", sdc_ppo_stats_launch(SdcPpoStats{sdc_ppo_blocks(n), (double)n, h->value_loss_part, stats}, st));
}

int sdc_value_loss(sdc_handle* h, long long n, const float* raw_values, const float* value_preds, const float* returns, double target_scale,
                   double target_shift, double clip_param, double huber_delta, int flags, double coef, float* loss, float* dvalue,
                   double* stats, void* stream) {
  if (refused(sdc_value_loss_refused(call_facts(h), n, raw_values, value_preds, returns, target_scale, target_shift, clip_param, huber_delta,
                                     flags, coef, loss, dvalue, stats)))
    return -2;
  return value_loss(h, n, raw_values, value_preds, returns, target_scale, target_shift, nullptr, clip_param, huber_delta, flags, coef, loss,
                    dvalue, stats, stream);
}

int sdc_critic_backward(sdc_handle* h, const float* share_obs, long long n_rows, const float* dvalue, float* grads, double* grad_sq,
                        void* stream) {
  if (refused(sdc_critic_backward_refused(call_facts(h), share_obs, n_rows, dvalue, grads, grad_sq))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SdcCriticGrad P;
  std::memset(&P, 0, sizeof(P));
  P.critic = critic_dev(h);
  P.critic_t = h->critic.pack_as<SdcCriticGradDev>(SDC_CRITIC_PACK_GRAD);
  P.rows = share_obs;
  P.n_rows = n_rows;
  P.dvalue = dvalue;
  return net_backward(h, &h->critic, 1, h->critic, P, "sdc_critic_grad_kernel", sdc_critic_grad_launch, "sdc_critic_grad_reduce_kernel",
                      sdc_critic_grad_reduce_launch, "sdc_critic_grad_sq_kernel", sdc_critic_grad_sq_launch, n_rows, grads, grad_sq, st);
}

int sdc_set_plan_critic(sdc_handle* h, double weight) {
  if (refused(sdc_set_plan_critic_refused(call_facts(h), weight))) return -2;
  h->plan_critic_weight = weight;
  return 0;
}

int sdc_get_plan_critic(const sdc_handle* h, double* weight) {
  if (!h || !weight) return fail_msg("sdc_get_plan_critic: null handle or out");
  *weight = h->plan_critic_weight;
  return 0;
}

// ---- the optimiser step (sdc_optim.hip) ------------------------------------------------------------------------------------------------
// The contract and the arithmetic: include/sustaindc_hip.h THE OPTIMISER STEP; the kernel's plan: sdc_optim_dev.hpp.
static int net_adam_step(sdc_handle* h, const SdcNet& n, const float* grads, const sdc_adam* adam, double* grad_norm, void* stream) {
  HIP_TRY(hipSetDevice(h->device));
  h->last_step_kernel = "sdc_adam_gather_kernel";
  return launched("sdc_adam_update_kernel / sdc_adam_gather_kernel",
                  sdc_adam_step_launch(sdc_net_adam_plan(n, grads, *adam, grad_norm), reinterpret_cast<hipStream_t>(stream)));
}
int sdc_actor_adam_step(sdc_handle* h, int agent_slot, const float* grads, const sdc_adam* adam, double* grad_norm, void* stream) {
  if (refused(sdc_adam_step_refused("sdc_actor_adam_step", call_facts(h), true, agent_slot, grads, adam, grad_norm))) return -2;
  return net_adam_step(h, h->actor[agent_slot], grads, adam, grad_norm, stream);
}
int sdc_critic_adam_step(sdc_handle* h, const float* grads, const sdc_adam* adam, double* grad_norm, void* stream) {
  if (refused(sdc_adam_step_refused("sdc_critic_adam_step", call_facts(h), false, -1, grads, adam, grad_norm))) return -2;
  return net_adam_step(h, h->critic, grads, adam, grad_norm, stream);
}

// the master parameters of a network -> the leading floats of its params struct (the device is waited for)
static int net_params_get(sdc_handle* h, const SdcNet& n, void* out) {
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, n.params, sizeof(float) * n.n_params, hipMemcpyDeviceToHost));
  return 0;
}
// the critic's scale and shift now: the ValueNorm block's while one is installed (one device read: sdc_value_norm_update moves them
// without the host), else the host record
static int critic_norm_now(sdc_handle* h, float* scale, float* shift) {
  SdcValueNormDev vn{};
  vn.scale = h->critic_scale, vn.shift = h->critic_shift;
  if (h->value_norm_installed) HIP_TRY(hipMemcpy(&vn, h->value_norm, sizeof(vn), hipMemcpyDeviceToHost));
  *scale = vn.scale, *shift = vn.shift;
  return 0;
}

int sdc_get_actor(sdc_handle* h, int agent_slot, sdc_actor_params* out) {
  if (refused(sdc_optim_get_refused("sdc_get_actor", call_facts(h), true, agent_slot, out != nullptr))) return -2;
  const SdcNet& n = h->actor[agent_slot];
  if (net_params_get(h, n, out) != 0) return -1;
  out->use_feature_normalization = n.feature_norm ? 1 : 0;
  out->activation = n.activation;
  return 0;
}

int sdc_get_critic(sdc_handle* h, sdc_critic_params* out) {
  if (refused(sdc_optim_get_refused("sdc_get_critic", call_facts(h), false, -1, out != nullptr))) return -2;
  if (net_params_get(h, h->critic, out) != 0) return -1;
  out->flags = h->critic_flags;
  return critic_norm_now(h, &out->scale, &out->shift);
}

// the moments and the state block of one network <-> host memory (the device is waited for)
static int net_optim_get(sdc_handle* h, const SdcNet& n, float* m, float* v, sdc_optim_state* st) {
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(m, n.m, n.n_params * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(v, n.v, n.n_params * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(st, n.state, sizeof(*st), hipMemcpyDeviceToHost));
  return 0;
}
static int net_optim_put(sdc_handle* h, const SdcNet& n, const float* m, const float* v, const sdc_optim_state* st) {
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(n.m, m, n.n_params * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(n.v, v, n.n_params * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(n.state, st, sizeof(*st), hipMemcpyHostToDevice));
  return 0;
}

int sdc_get_actor_optim(sdc_handle* h, int agent_slot, float* m, float* v, sdc_optim_state* st) {
  if (refused(sdc_optim_get_refused("sdc_get_actor_optim", call_facts(h), true, agent_slot, m && v && st))) return -2;
  return net_optim_get(h, h->actor[agent_slot], m, v, st);
}
int sdc_set_actor_optim(sdc_handle* h, int agent_slot, const float* m, const float* v, const sdc_optim_state* st) {
  if (refused(sdc_set_optim_refused("sdc_set_actor_optim", call_facts(h), true, agent_slot, m, v, st))) return -2;
  return net_optim_put(h, h->actor[agent_slot], m, v, st);
}
int sdc_get_critic_optim(sdc_handle* h, float* m, float* v, sdc_optim_state* st) {
  if (refused(sdc_optim_get_refused("sdc_get_critic_optim", call_facts(h), false, -1, m && v && st))) return -2;
  return net_optim_get(h, h->critic, m, v, st);
}
int sdc_set_critic_optim(sdc_handle* h, const float* m, const float* v, const sdc_optim_state* st) {
  if (refused(sdc_set_optim_refused("sdc_set_critic_optim", call_facts(h), false, -1, m, v, st))) return -2;
  return net_optim_put(h, h->critic, m, v, st);
}

int sdc_set_critic_norm(sdc_handle* h, double scale, double shift, void* stream) {
  if (refused(sdc_set_critic_norm_refused(call_facts(h), scale, shift))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  h->critic_scale = (float)scale;
  h->critic_shift = (float)shift;
  h->value_norm_installed = false;      // (scale and shift set by hand: no running state)
  return launched("sdc_critic_norm_kernel",
                  sdc_critic_norm_launch(SdcCriticNorm{critic_dev(h), h->critic_scale, h->critic_shift}, reinterpret_cast<hipStream_t>(stream)));
}

// ---- train on the device (sdc_minibatch.hip) ---------------------------------------------------------------------------------------------
// The contract: include/sustaindc_hip.h TRAIN ON THE DEVICE; the arithmetic: sdc_minibatch.hpp; the kernels' plans: sdc_minibatch_dev.hpp.
int sdc_permutation(sdc_handle* h, long long n, uint64_t seed, uint64_t stream_id, int32_t* perm, void* stream) {
  if (refused(sdc_permutation_refused(call_facts(h), n, perm))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  return launched("sdc_permutation_kernel",
                  sdc_permutation_launch(SdcPermutation{sdc_perm_key(n, seed, stream_id), perm}, reinterpret_cast<hipStream_t>(stream)));
}

int sdc_gather_rows(sdc_handle* h, const int32_t* idx, long long n_rows, long long n_src_rows, const sdc_gather_segment* segs, int n_segs,
                    int32_t* bad, void* stream) {
  if (refused(sdc_gather_rows_refused(call_facts(h), idx, n_rows, n_src_rows, segs, n_segs, bad))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  SdcGatherRows P;
  std::memset(&P, 0, sizeof(P));
  P.idx = idx;
  P.n_rows = n_rows;
  P.n_src_rows = (unsigned)n_src_rows;
  P.n_segs = n_segs;
  P.bad = bad;
  long long first = 0;
  for (int g = 0; g < n_segs; g++) {
    P.seg[g] = SdcGatherSeg{static_cast<const uint32_t*>(segs[g].src), static_cast<uint32_t*>(segs[g].dst), segs[g].src_stride,
                            segs[g].dst_stride, (int)first, segs[g].n_dwords};
    first += segs[g].n_dwords;
  }
  if (first > 0x7fffffffll) return fail_msg("sdc_gather_rows: the segments' n_dwords add up to more than 2147483647");
  P.row_dwords = (int)first;
  return launched("sdc_gather_rows_kernel", sdc_gather_rows_launch(P, reinterpret_cast<hipStream_t>(stream)));
}

int sdc_set_value_norm(sdc_handle* h, const sdc_value_norm* st) {
  if (refused(sdc_set_value_norm_refused(call_facts(h), st))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  SdcValueNormDev vn{};
  if (!st) {      // uninstall: the critic keeps the scale and shift it has, and the host record follows them
    if (critic_norm_now(h, &h->critic_scale, &h->critic_shift) != 0) return -1;
    h->value_norm_installed = false;
    return 0;
  }
  vn.running_mean = st->running_mean;
  vn.running_mean_sq = st->running_mean_sq;
  vn.debiasing_term = st->debiasing_term;
  sdc_value_norm_derive(vn);
  HIP_TRY(hipMemcpy(h->value_norm, &vn, sizeof(vn), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(&critic_dev(h)->scale, &vn.scale, sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(&critic_dev(h)->shift, &vn.shift, sizeof(float), hipMemcpyHostToDevice));
  h->critic_scale = vn.scale;
  h->critic_shift = vn.shift;
  h->value_norm_installed = true;
  return 0;
}

int sdc_get_value_norm(sdc_handle* h, sdc_value_norm* out) {
  if (refused(sdc_get_value_norm_refused(call_facts(h), h && h->value_norm_installed, out))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  SdcValueNormDev vn;
  HIP_TRY(hipMemcpy(&vn, h->value_norm, sizeof(vn), hipMemcpyDeviceToHost));
  *out = sdc_value_norm{vn.running_mean, vn.running_mean_sq, vn.debiasing_term};
  return 0;
}

int sdc_value_norm_update(sdc_handle* h, const float* returns, long long n, double beta, void* stream) {
  if (refused(sdc_value_norm_update_refused(call_facts(h), h && h->value_norm_installed, returns, n, beta))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  if (!h->value_norm_part && dev_alloc(h, &h->value_norm_part, (size_t)SDC_VN_MAX_BLOCKS * 2, false) != 0) return -1;
  const int B = sdc_value_norm_blocks(n);
  return launched("sdc_value_norm_sums_kernel / sdc_value_norm_update_kernel",
                  sdc_value_norm_update_launch(SdcValueNormSums{returns, n, h->value_norm_part},
                                               SdcValueNormUpdate{B, n, beta, h->value_norm_part, h->value_norm, critic_dev(h)},
                                               reinterpret_cast<hipStream_t>(stream)));
}

int sdc_value_loss_normed(sdc_handle* h, long long n, const float* raw_values, const float* value_preds, const float* returns,
                          double clip_param, double huber_delta, int flags, double coef, float* loss, float* dvalue, double* stats,
                          void* stream) {
  if (refused(sdc_value_loss_normed_refused(call_facts(h), h && h->value_norm_installed, n, raw_values, value_preds, returns, clip_param,
                                            huber_delta, flags, coef, loss, dvalue, stats)))
    return -2;
  return value_loss(h, n, raw_values, value_preds, returns, 0.0, 0.0, h->value_norm, clip_param, huber_delta, flags, coef, loss, dvalue, stats,
                    stream);
}

// ---- plan with the cross-entropy method (sdc_cem.hip, sdc_cem_groups.hip) -----------------------------------------------------------
// The contract and the arithmetic: include/sustaindc_hip.h; the kernels' plans: sdc_cem.hpp, sdc_cem_groups.hpp.

extern "C++" {
// the fields the per-env and the group kernels' plans share, from the fields the two parameter structs share
template <class Sample, class Params>
static Sample cem_sample_plan(const int n_envs, const int n_steps, const Params& c, const double* probs, const int32_t* best_seq, int32_t* cand) {
  Sample Q;
  std::memset(&Q, 0, sizeof(Q));
  Q.n_envs = n_envs;
  Q.n_steps = n_steps;
  Q.draw = c.draw;
  Q.key0 = (unsigned)c.seed;
  Q.key1 = (unsigned)(c.seed >> 32);
  Q.probs = probs;
  Q.best_seq = best_seq;
  Q.cand = cand;
  for (int a = 0; a < 3; a++) Q.fixed[a] = c.fixed_action[a];
  return Q;
}
template <class Refit, class Params>
static Refit cem_refit_plan(const int n_envs, const int n_steps, const Params& c, const double* score, const int32_t* cand, double* probs,
                            int32_t* best_seq, int32_t* best_action) {
  Refit F;
  std::memset(&F, 0, sizeof(F));
  F.n_envs = n_envs;
  F.n_steps = n_steps;
  F.n_elite = c.n_elite;
  F.alpha = c.alpha;
  F.take = 1.0 - c.alpha;
  F.p_min = c.p_min;
  F.score = score;
  F.cand = cand;
  F.probs = probs;
  F.best_seq = best_seq;
  F.best_action = best_action;
  for (int a = 0; a < 3; a++) F.fixed[a] = c.fixed_action[a];
  return F;
}

// The iterations of a CEM call: the sample launch of plan Q with the iteration's counter word, the rollouts of the n_cand candidate
// arrays in `cand` (plan_candidates), the refit launch of plan F with the iteration's row of best_score, `stride` entries long
template <class Sample, class Refit>
static int cem_iterations(PlanSession& P, const int n_iters, const int iter0, const int n_cand, const int32_t* cand, double* cand_score,
                          double* best_score, const size_t stride, Sample& Q, hipError_t (*sample)(const Sample&, hipStream_t),
                          const char* sample_kernel, Refit& F, hipError_t (*refit)(const Refit&, hipStream_t), const char* refit_kernel) {
  int rc = 0;
  for (int i = 0; i < n_iters && rc == 0; i++) {
    Q.c3 = ((unsigned)(iter0 + i) << 16) | SDC_CEM_STREAM;
    rc = launched(sample_kernel, sample(Q, P.st()));
    if (rc == 0) rc = plan_candidates(P, n_cand, cand, nullptr, cand_score);
    if (rc == 0) {
      F.last = i == n_iters - 1;
      F.best_score = best_score + (size_t)i * stride;
      rc = launched(refit_kernel, refit(F, P.st()));
    }
  }
  return rc;
}

// The per-env planner's body for a plan of K steps, as plan_marked takes it: (session) -> rc, which enqueues the iterations of c over
// the caller's arrays.  sdc_plan_cem runs it once, sdc_rollout_cem_stats per planned decision with that decision's draw in c.
static auto cem_body(const sdc_handle* h, const sdc_cem_params& c, const int K, double* probs, int32_t* best_seq, double* best_score,
                     int32_t* best_action, int32_t* cand, double* cand_score) {
  const int N = h->cfg.n_envs, n_iters = c.n_iters, iter0 = c.iter0, n_cand = c.n_cand;
  SdcCemSample Q = cem_sample_plan<SdcCemSample>(N, K, c, probs, best_seq, cand);
  Q.n_cand = n_cand;
  Q.env_base = h->cfg.env_index_base;
  SdcCemRefit T = cem_refit_plan<SdcCemRefit>(N, K, c, cand_score, cand, probs, best_seq, best_action);
  T.n_cand = n_cand;
  return [=](PlanSession& P) mutable {
    return cem_iterations(P, n_iters, iter0, n_cand, cand, cand_score, best_score, (size_t)N, Q, sdc_cem_sample_launch,
                          "sdc_cem_sample_kernel", T, sdc_cem_refit_launch, "sdc_cem_refit_kernel");
  };
}

// ... and the groups planner's, the candidates in env slots: per iteration ONE rollout of the whole batch (plan_candidates with the
// single "candidate" cand) between the group sample and the group refit kernel.  sdc_plan_cem_groups, sdc_rollout_cem_groups_stats.
static auto cem_groups_body(const sdc_handle* h, const sdc_cem_group_params& c, const int K, double* probs, int32_t* best_seq,
                            double* best_score, int32_t* best_action, int32_t* step_actions, int32_t* cand, double* cand_score) {
  const int N = h->cfg.n_envs, G = N / c.group_size, n_iters = c.n_iters, iter0 = c.iter0;
  SdcCemGroupSample Q = cem_sample_plan<SdcCemGroupSample>(N, K, c, probs, best_seq, cand);
  SdcCemGroupRefit T = cem_refit_plan<SdcCemGroupRefit>(N, K, c, cand_score, cand, probs, best_seq, best_action);
  Q.group_size = T.group_size = c.group_size;
  Q.n_groups = T.n_groups = G;
  Q.group_base = c.group_base;
  T.step_actions = step_actions;
  return [=](PlanSession& P) mutable {
    return cem_iterations(P, n_iters, iter0, 1, cand, cand_score, best_score, (size_t)G, Q, sdc_cem_group_sample_launch,
                          "sdc_cem_group_sample_kernel", T, sdc_cem_group_refit_launch, "sdc_cem_group_refit_kernel");
  };
}
}  // extern "C++"

int sdc_plan_cem(sdc_handle* h, int n_steps, const sdc_cem_params* cem, const sdc_plan_objective* objective, double* probs,
                 int32_t* best_seq, double* best_score, int32_t* best_action, int32_t* cand, double* cand_score, float* obs,
                 float* share_obs, void* stream) {
  sdc_plan_objective obj;
  if (refused(sdc_plan_cem_refused(call_facts(h), n_steps, cem, objective, probs, best_seq, best_score, best_action, cand, cand_score, obs,
                                   share_obs, obj)))
    return -2;
  const sdc_cem_params c = *cem;
  return plan_session(h, n_steps, obj, obs, share_obs, stream,
                      cem_body(h, c, n_steps, probs, best_seq, best_score, best_action, cand, cand_score));
}

// sdc_plan_cem with the candidates in env slots (cem_groups_body)
int sdc_plan_cem_groups(sdc_handle* h, int n_steps, const sdc_cem_group_params* cem, const sdc_plan_objective* objective, double* probs,
                        int32_t* best_seq, double* best_score, int32_t* best_action, int32_t* step_actions, int32_t* cand,
                        double* cand_score, float* obs, float* share_obs, void* stream) {
  sdc_plan_objective obj;
  if (refused(sdc_plan_cem_groups_refused(call_facts(h), n_steps, cem, objective, probs, best_seq, best_score, best_action, step_actions, cand,
                                          cand_score, obs, share_obs, obj)))
    return -2;
  const sdc_cem_group_params c = *cem;
  return plan_session(h, n_steps, obj, obs, share_obs, stream,
                      cem_groups_body(h, c, n_steps, probs, best_seq, best_score, best_action, step_actions, cand, cand_score));
}

// ---- episode statistics (sdc_stats.hip, sdc_policy_stats.hip) ---------------------------------------------------------------------
// The contracts and the arithmetic: include/sustaindc_hip.h; the kernels' plans and the lane mappings: sdc_stats.hpp,
// sdc_policy_stats.hpp.  The rollouts go into the plan calls' output block (plan_out_block, rollout_chunks); nothing is marked or rewound.

using StatsArrays = SdcStatsArrays;      // (the caller's arrays of the statistics calls: sdc_refusals.hpp)

// sdc_stats_reduce_kernel's plan over the block (layout B) into the caller's arrays, but for the chunk's steps and init
static SdcStatsReduce stats_reduce_plan(const sdc_handle* h, const SdcPlanBlock& B, const StatsArrays& a) {
  unsigned char* const out = h->plan_out;
  SdcStatsReduce S;
  std::memset(&S, 0, sizeof(S));
  S.n_envs = h->cfg.n_envs;
  S.rew = reinterpret_cast<const float*>(out + B.rew);
  S.info = reinterpret_cast<const float*>(out + B.info);
  S.stats = a.stats;
  S.returns = a.returns;
  S.counts = a.counts;
  return S;
}

// sdc_stats_last_kernel behind a call's last chunk of last_steps steps in the block (layout B): its LAST step's slices -> the caller's
// single-step arrays
static int stats_last(const sdc_handle* h, const SdcPlanBlock& B, const int last_steps, const StatsArrays& a, hipStream_t st) {
  const size_t N = (size_t)h->cfg.n_envs;
  unsigned char* const out = h->plan_out;
  const size_t last = (size_t)(last_steps - 1) * N;
  SdcStatsLast Q;
  std::memset(&Q, 0, sizeof(Q));
  Q.n_envs = (int)N;
  Q.obs = reinterpret_cast<const float*>(out + B.obs) + last * SDC_OBS_OUT;
  Q.share_obs = reinterpret_cast<const float*>(out + B.share_obs) + last * SDC_SHARE_OBS_DIM;
  Q.rew = reinterpret_cast<const float*>(out + B.rew) + last * SDC_N_AGENTS;
  Q.info = reinterpret_cast<const float*>(out + B.info) + last * SDC_INFO_DIM;
  Q.done = out + B.done + last;
  Q.final_obs = reinterpret_cast<const float*>(out + B.final_obs);
  Q.o_obs = a.obs;
  Q.o_share_obs = a.share_obs;
  Q.o_rew = a.rew;
  Q.o_info = a.info;
  Q.o_done = a.done;
  Q.o_final_obs = a.final_obs;
  return launched("sdc_stats_last_kernel", sdc_stats_last_launch(Q, st));
}

// The chunks of a statistics call, the block (layout B, of `chunk` steps) grown already: rollout (rollout_chunks'), behind each chunk
// sdc_stats_reduce_kernel and extra(first step, steps, init) -> rc; behind the last chunk sdc_stats_last_kernel
extern "C++" {
template <class Rollout, class Extra>
static int stats_chunks(sdc_handle* h, const SdcPlanBlock& B, const int n_steps, const int chunk, const int accumulate, const StatsArrays& a,
                        hipStream_t st, Rollout&& rollout, Extra&& extra) {
  SdcStatsReduce S = stats_reduce_plan(h, B, a);
  int last_steps = 0;
  const int rc = rollout_chunks(h, B, n_steps, chunk, rollout, [&](const int k0, const int steps) {
    S.steps = last_steps = steps;
    S.init = (k0 == 0 && accumulate == 0) ? 1 : 0;
    const int r = launched("sdc_stats_reduce_kernel", sdc_stats_reduce_launch(S, st));
    return r ? r : extra(k0, steps, S.init);
  });
  return rc ? rc : stats_last(h, B, last_steps, a, st);
}
}  // extern "C++"

int sdc_rollout_stats(sdc_handle* h, int n_steps, const int32_t* actions, int accumulate, double* stats, double* returns,
                      int32_t* counts, float* obs, float* share_obs, float* rew, uint8_t* done, float* info, float* final_obs,
                      void* stream) {
  const StatsArrays a = {stats, returns, counts, obs, share_obs, rew, done, info, final_obs};
  if (refused(sdc_rollout_stats_refused(call_facts(h), n_steps, actions, accumulate, a))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  int chunk;
  SdcPlanBlock B;
  if (plan_out_block(h, n_steps, chunk, B)) return -1;
  return stats_chunks(h, B, n_steps, chunk, accumulate, a, reinterpret_cast<hipStream_t>(stream), rollout_of(h, actions, stream),
                      [](int, int, int) { return 0; });
}

int sdc_rollout_actor_stats(sdc_handle* h, int n_steps, int sample, int accumulate, double* stats, double* returns, int32_t* counts,
                            int32_t* policy_counts, double* policy_sums, float* obs, float* share_obs, float* rew, uint8_t* done,
                            float* info, float* final_obs, void* stream) {
  const StatsArrays a = {stats, returns, counts, obs, share_obs, rew, done, info, final_obs};
  // (what sdc_rollout_actor would refuse about the actors and the batch is asked before anything is enqueued; its own checks stay where
  // they are: every chunk passes them again.  The output arrays are the handle's block's: all there, 256-byte aligned)
  SdcCallFacts facts = call_facts(h);
  if (h) {
    facts.step = step_facts(h, true, nullptr, nullptr, nullptr, nullptr, nullptr, false);
    facts.step.share_obs = facts.step.info = facts.step.actions_out = true;
  }
  if (refused(sdc_rollout_actor_stats_refused(facts, n_steps, sample, accumulate, a, policy_counts, policy_sums))) return -2;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t N = (size_t)h->cfg.n_envs;
  int chunk;
  SdcPlanBlock B;
  if (plan_out_block(h, n_steps, chunk, B)) return -1;
  const SdcPolicyBlock PB = sdc_policy_block(N, (size_t)chunk);
  if (plan_grow(&h->policy_out, &h->policy_out_bytes, PB.bytes)) return -1;
  SdcPolicyStats P;
  std::memset(&P, 0, sizeof(P));
  P.n_envs = (int)N;
  P.actions = reinterpret_cast<const int32_t*>(h->policy_out + PB.actions);
  P.logits = reinterpret_cast<const float*>(h->policy_out + PB.logits);
  P.counts = policy_counts;
  P.sums = policy_sums;
  int32_t* const actions_out = reinterpret_cast<int32_t*>(h->policy_out + PB.actions);
  float* const logits_out = reinterpret_cast<float*>(h->policy_out + PB.logits);
  return stats_chunks(
      h, B, n_steps, chunk, accumulate, a, st,
      [=](int, const int steps, float* b_obs, float* b_share_obs, float* b_rew, uint8_t* b_done, float* b_info, float* b_final_obs) {
        return sdc_rollout_actor(h, steps, sample, b_obs, b_share_obs, b_rew, b_done, b_info, b_final_obs, actions_out,
                                 policy_counts ? logits_out : nullptr, stream);
      },
      [&](int, const int steps, const int init) {
        if (!policy_counts) return 0;
        P.steps = steps;
        P.init = init;
        return launched("sdc_policy_stats_kernel", sdc_policy_stats_launch(P, st));
      });
}

// ---- planner evaluation (sdc_mpc.hip) -----------------------------------------------------------------------------------------------
// The contract: include/sustaindc_hip.h; the decision schedule: sdc_mpc_schedule.hpp; the two kernels' plans: sdc_mpc.hpp.  A planned
// decision is sdc_plan_cem's own body (plan_marked around cem_body), the step sdc_rollout_stats' with a one-step chunk; the
// discount table of the longest horizon is staged once, and every decision reads its prefix.  sdc_rollout_cem_groups_stats
// (sdc_mpc_groups.hip) is the same loop (mpc_steps) with sdc_plan_cem_groups' body (cem_groups_body) and its own fold kernel, a sync in
// front and the agreement check behind the step.

extern "C++" {
// what the two fold kernels' plans share but for the decision's own fields and the idle actions (mpc_steps); best_score's rows are `row`
// entries long (N, or G)
template <class Fold>
static Fold mpc_fold_plan(const int n_envs, const size_t row, const int n_iters, const double* best_score, int32_t* best_action,
                          int32_t* plan_counts, double* plan_sums) {
  Fold F;
  std::memset(&F, 0, sizeof(F));
  F.n_envs = n_envs;
  F.best_action = best_action;
  F.counts = plan_counts;
  F.sums = plan_sums;
  F.score_first = best_score;
  F.score_last = best_score + (size_t)(n_iters - 1) * row;
  return F;
}

// The steps of a planner evaluation once its arguments have passed.  m: the loop's fields (sdc_mpc_params or sdc_mpc_group_params);
// k_max: the longest planned decision (sdc_refusals.hpp sdc_mpc_longest).  Every buffer at its largest before anything is enqueued: the
// step's one-step block, the longest decision's (k_max steps) rows, block and forecast; then first() -> rc (the groups' sync); the
// discount table of H steps staged once; then per step the schedule's decision d -- planned: sdc_mpc_start_kernel (plan A, of which the caller fills n_envs, probs and best_seq) and plan_marked
// around body(d), the planner's body for that decision (cem_body, cem_groups_body) --, the fold kernel (plan F through `fold`; a planned
// decision without statistics has nothing to fold), and the step: sdc_rollout_stats' path with a one-step chunk and `actions` [N][3],
// behind its reduce kernel behind(B1, init) -> rc.  Behind the last step sdc_stats_last_kernel.  The idle actions go into A and F here.
template <class Params, class Fold, class First, class Body, class Behind>
static int mpc_steps(sdc_handle* h, const int n_steps, const Params& m, const int k_max, const int accumulate,
                     const sdc_plan_objective& obj, const StatsArrays& a, SdcMpcStart A, Fold F, hipError_t (*fold)(const Fold&, hipStream_t),
                     const char* fold_kernel, const int32_t* actions, void* stream, First&& first, Body&& body, Behind&& behind) {
  const int H = m.horizon, warm_start = m.warm_start, resume_steps = m.resume ? m.resume_steps : 0, auto_reset = h->cfg.auto_reset ? 1 : 0;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int k = 0; k < 3; k++) A.idle[k] = F.idle[k] = m.idle_action[k];
  int chunk1;
  SdcPlanBlock B1;
  if (plan_out_block(h, 1, chunk1, B1)) return -1;
  SdcForecastSwap W;
  std::memset(&W, 0, sizeof(W));
  if (k_max > 0) {
    PlanRun R;
    if (plan_prepare(h, k_max, obj, R) || plan_forecast_swap(h, k_max, W)) return -1;
  }
  if (const int rc = first()) return rc;

  void* pin = nullptr;
  if (stage_acquire(h, h->plan_stage, &pin)) return -1;
  double* const g = static_cast<double*>(pin);
  g[0] = 1.0;
  for (int k = 1; k < H; k++) g[k] = g[k - 1] * obj.gamma;
  int rc = 0;
  const int staged = stage_commit(h, h->plan_stage, (size_t)H, st, [&](const void* g_dev) {
    SdcMpcSchedule S(H, warm_start, auto_reset, resume_steps);
    SdcStatsReduce R1 = stats_reduce_plan(h, B1, a);
    R1.steps = 1;
    for (int t = 0; t < n_steps && rc == 0; t++) {
      const SdcMpcDecision d = S.next(h->mirror.steps_to_terminal());
      const int init = (t == 0 && accumulate == 0) ? 1 : 0;
      if (d.planned) {
        const int K = d.steps;
        A.steps = K;
        A.fresh = d.fresh;
        rc = launched("sdc_mpc_start_kernel", sdc_mpc_start_launch(A, st));
        PlanSession P{h, {}, g_dev, g[K - 1] * obj.gamma, a.obs, a.share_obs, stream};
        if (rc == 0 && (plan_prepare(h, K, obj, P.R) || plan_forecast_swap(h, K, W))) rc = -1;
        if (rc == 0) rc = plan_marked(P, W, body(d));
      }
      if (rc == 0 && (!d.planned || F.counts)) {
        F.planned = d.planned;
        F.init = init;
        rc = launched(fold_kernel, fold(F, st));
      }
      if (rc == 0)
        rc = rollout_chunks(h, B1, 1, 1, rollout_of(h, actions, stream), [&](int, int) {
          R1.init = init;
          const int r = launched("sdc_stats_reduce_kernel", sdc_stats_reduce_launch(R1, st));
          return r ? r : behind(B1, init);
        });
    }
    if (rc == 0) rc = stats_last(h, B1, 1, a, st);
    return hipSuccess;
  });
  return rc ? rc : staged;
}
}  // extern "C++"

int sdc_rollout_cem_stats(sdc_handle* h, int n_steps, const sdc_mpc_params* mpc, const sdc_plan_objective* objective, int accumulate,
                          double* stats, double* returns, int32_t* counts, int32_t* plan_counts, double* plan_sums, double* probs,
                          int32_t* best_seq, double* best_score, int32_t* best_action, int32_t* cand, double* cand_score, float* obs,
                          float* share_obs, float* rew, uint8_t* done, float* info, float* final_obs, void* stream) {
  const StatsArrays a = {stats, returns, counts, obs, share_obs, rew, done, info, final_obs};
  sdc_plan_objective obj;
  int k_max = 0;
  if (refused(sdc_rollout_cem_stats_refused(call_facts(h), n_steps, mpc, objective, accumulate, a, plan_counts, plan_sums, probs, best_seq,
                                            best_score, best_action, cand, cand_score, obj, k_max)))
    return -2;
  const sdc_mpc_params m = *mpc;
  const sdc_cem_params c = m.cem;
  const int N = h->cfg.n_envs;
  return mpc_steps(
      h, n_steps, m, k_max, accumulate, obj, a, SdcMpcStart{N, 0, 0, {}, probs, best_seq},
      mpc_fold_plan<SdcMpcFold>(N, (size_t)N, c.n_iters, best_score, best_action, plan_counts, plan_sums), sdc_mpc_fold_launch,
      "sdc_mpc_fold_kernel", best_action, stream, [] { return 0; },
      [&](const SdcMpcDecision& d) {
        sdc_cem_params ck = c;
        ck.draw = c.draw + d.draw_index;
        return cem_body(h, ck, d.steps, probs, best_seq, best_score, best_action, cand, cand_score);
      },
      [](const SdcPlanBlock&, int) { return 0; });
}

// sdc_rollout_cem_stats over replica groups: the loop above with sdc_plan_cem_groups' body (the group sample and group refit kernels, one
// rollout of the batch per iteration), sdc_mpc_start_kernel over the G groups, sdc_mpc_group_fold_kernel, the step played with
// step_actions, and sdc_group_agree_kernel behind the step's reduce.  sync_first: one sdc_clone_envs in front, the groups' first envs ->
// their replicas; the episode's end is then the first envs' (what the mirror says once the clone has been made).
int sdc_rollout_cem_groups_stats(sdc_handle* h, int n_steps, const sdc_mpc_group_params* mpc, const sdc_plan_objective* objective,
                                 int accumulate, double* stats, double* returns, int32_t* counts, int32_t* plan_counts, double* plan_sums,
                                 int32_t* diverged, double* probs, int32_t* best_seq, double* best_score, int32_t* best_action,
                                 int32_t* step_actions, int32_t* cand, double* cand_score, float* obs, float* share_obs, float* rew,
                                 uint8_t* done, float* info, float* final_obs, void* stream) {
  const StatsArrays a = {stats, returns, counts, obs, share_obs, rew, done, info, final_obs};
  sdc_plan_objective obj;
  int k_max = 0;
  if (refused(sdc_rollout_cem_groups_stats_refused(call_facts(h), n_steps, mpc, objective, accumulate, a, plan_counts, plan_sums, diverged,
                                                   probs, best_seq, best_score, best_action, step_actions, cand, cand_score, obj, k_max)))
    return -2;
  const sdc_mpc_group_params m = *mpc;
  const sdc_cem_group_params c = m.cem;
  const int N = h->cfg.n_envs, R = c.group_size, G = N / R;

  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SdcMpcGroupFold F = mpc_fold_plan<SdcMpcGroupFold>(N, (size_t)G, c.n_iters, best_score, best_action, plan_counts, plan_sums);
  F.n_groups = G;
  F.step_actions = step_actions;
  F.diverged = diverged;
  SdcGroupAgree Y;
  std::memset(&Y, 0, sizeof(Y));
  Y.n_envs = N;
  Y.group_size = R;
  Y.diverged = diverged;

  return mpc_steps(
      h, n_steps, m, k_max, accumulate, obj, a, SdcMpcStart{G, 0, 0, {}, probs, best_seq}, F,
      sdc_mpc_group_fold_launch, "sdc_mpc_group_fold_kernel", step_actions, stream,
      [&] {
        if (!m.sync_first) return 0;
        std::vector<int32_t> src((size_t)(N - G)), dst((size_t)(N - G));
        size_t k = 0;
        for (int e = 0; e < N; e++)
          if (e % R != 0) {
            src[k] = e - e % R;
            dst[k++] = e;
          }
        return sdc_clone_envs(h, src.data(), dst.data(), N - G, obs, share_obs, stream);
      },
      [&](const SdcMpcDecision& d) {
        sdc_cem_group_params ck = c;
        ck.draw = c.draw + d.draw_index;
        return cem_groups_body(h, ck, d.steps, probs, best_seq, best_score, best_action, step_actions, cand, cand_score);
      },
      [&](const SdcPlanBlock& B1, int) {
        if (!diverged) return 0;
        // (the one-step block: step 0's slices)
        Y.rew = reinterpret_cast<const float*>(h->plan_out + B1.rew);
        Y.info = reinterpret_cast<const float*>(h->plan_out + B1.info);
        Y.done = h->plan_out + B1.done;
        return launched("sdc_group_agree_kernel", sdc_group_agree_launch(Y, st));
      });
}

}  // extern "C"
