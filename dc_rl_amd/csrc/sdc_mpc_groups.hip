// sdc_mpc_groups.hip -- sdc_mpc_group_fold_kernel and sdc_group_agree_kernel: what happens between two decisions of
// sdc_rollout_cem_groups_stats and the check of the replicas behind its step (sdc_capi.hip; the plans, the lane mappings and the address
// bounds: sdc_mpc_groups.hpp; the schedule: sdc_mpc_schedule.hpp; the kernel in front of a planned decision: sdc_mpc.hip's start kernel).
//
// The fold's arithmetic is the one include/sustaindc_hip.h states for sdc_rollout_cem_stats, per group: integer counts, and per group two
// fp64 additions and one fp64 subtraction per planned decision, no fused operation possible (the pragma below says it for this file
// whatever the flags).  The agreement check is integer throughout: exclusive-ors of the rows' bits and an integer atomic add.
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_mpc_groups.hpp"
#include "sdc_rowcopy.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int ROW_UNITS = SDC_INFO_DIM / 4;          // 16-byte units per info row
constexpr int REW_LANE = ROW_UNITS;                  // the lane of a row that takes rew and done
constexpr int RSV_UNIT = SDC_INFO_RESERVED / 4;      // the lane that owns info[reserved] ...
constexpr int RSV_DWORD = SDC_INFO_RESERVED % 4;     // ... and the column's place in its unit
static_assert(SDC_MPCG_BLOCK % SDC_WAVE == 0 && SDC_MPCG_AGREE_BLOCK % SDC_WAVE == 0, "whole wavefronts per workgroup");
static_assert(SDC_WAVE == 64 && SDC_WAVE % SDC_MPCG_AGREE_ROW == 0, "whole rows per wavefront, a ballot of 64 lanes");
static_assert(SDC_INFO_DIM % 4 == 0 && ROW_UNITS < SDC_MPCG_AGREE_ROW, "an info row is whole 16-byte units, and a row of lanes has one to spare");
static_assert(RSV_DWORD == 3, "the agree kernel clears the unit's fourth dword");
static_assert(SDC_POLICY_COUNTS == 5 && SDC_POLICY_N0 == 0 && SDC_POLICY_N1 == 1 && SDC_POLICY_N2 == 2 && SDC_POLICY_SWITCHES == 3 &&
                  SDC_POLICY_LAST == 4,
              "the counts");
static_assert(SDC_PLAN_SUMS == 4 && SDC_PLAN_SCORE == 0 && SDC_PLAN_GAIN == 1 && SDC_PLAN_PLANNED == 2 && SDC_PLAN_IDLE == 3, "the sums");

typedef double f64x2 __attribute__((ext_vector_type(2)));

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_MPCG_BLOCK) sdc_mpc_group_fold_kernel(SdcMpcGroupFold P) {
  const size_t glanes = (size_t)P.n_groups * SDC_N_AGENTS, elanes = (size_t)P.n_envs * SDC_N_AGENTS;
  const size_t t = (size_t)blockIdx.x * SDC_MPCG_BLOCK + threadIdx.x;
  const int a = (int)(t % SDC_N_AGENTS);
  const int idle = a == 0 ? P.idle[0] : (a == 1 ? P.idle[1] : P.idle[2]);
  // an idle decision: every env's row of step_actions, a dword per lane
  if (!P.planned && t < elanes) P.step_actions[t] = idle;
  if (t >= glanes) return;      // (no barrier below: the lanes past the groups' leave)
  const size_t g = t / SDC_N_AGENTS;
  int j;
  if (P.planned) {
    j = P.best_action[t];
  } else {
    j = idle;
    P.best_action[t] = j;
  }
  if (!P.counts) return;

  int32_t* const cnt = P.counts + t * SDC_POLICY_COUNTS;
  int n0 = 0, n1 = 0, n2 = 0, switches = 0, last = -1;
  if (!P.init) {
    n0 = cnt[SDC_POLICY_N0];
    n1 = cnt[SDC_POLICY_N1];
    n2 = cnt[SDC_POLICY_N2];
    switches = cnt[SDC_POLICY_SWITCHES];
    last = cnt[SDC_POLICY_LAST];
  }
  n0 += j == 0 ? 1 : 0;
  n1 += j == 1 ? 1 : 0;
  n2 += j == 2 ? 1 : 0;
  switches += (last >= 0 && j != last) ? 1 : 0;
  cnt[SDC_POLICY_N0] = n0;
  cnt[SDC_POLICY_N1] = n1;
  cnt[SDC_POLICY_N2] = n2;
  cnt[SDC_POLICY_SWITCHES] = switches;
  cnt[SDC_POLICY_LAST] = j;

  if (a != 0) return;
  if (P.init) P.diverged[g] = 0;
  // the group's row of sums: SCORE, GAIN | PLANNED, IDLE
  f64x2* const sums = reinterpret_cast<f64x2*>(P.sums + g * SDC_PLAN_SUMS);
  f64x2 sg = {0.0, 0.0}, pi = {0.0, 0.0};
  if (!P.init) {
    sg = sums[0];
    pi = sums[1];
  }
  if (P.planned) {
    const double s_first = P.score_first[g], s_last = P.score_last[g];
    sg.x += s_last;
    sg.y += s_last - s_first;
    pi.x += 1.0;
  } else {
    pi.y += 1.0;
  }
  sums[0] = sg;
  sums[1] = pi;
}

// Every lane of a wavefront reaches the ballot: a lane with nothing to compare votes "equal".
extern "C" __global__ void __launch_bounds__(SDC_MPCG_AGREE_BLOCK) sdc_group_agree_kernel(SdcGroupAgree P) {
  const int N = P.n_envs, R = P.group_size;
  const int t = (int)blockIdx.x * SDC_MPCG_AGREE_BLOCK + (int)threadIdx.x;
  const int env = t / SDC_MPCG_AGREE_ROW, u = t % SDC_MPCG_AGREE_ROW;
  const int lead = env - env % R;
  const bool replica = env < N && env != lead;
  bool differs = false;
  if (replica && u < ROW_UNITS) {
    const u32x4* const ip = reinterpret_cast<const u32x4*>(P.info);
    u32x4 d = ip[(size_t)env * ROW_UNITS + (size_t)u] ^ ip[(size_t)lead * ROW_UNITS + (size_t)u];
    if (u == RSV_UNIT) d.w = 0u;      // info[reserved] says how the step was served, not what it computed
    differs = (d.x | d.y | d.z | d.w) != 0u;
  } else if (replica && u == REW_LANE) {
    const unsigned* const mine = reinterpret_cast<const unsigned*>(P.rew) + (size_t)env * SDC_N_AGENTS;
    const unsigned* const his = reinterpret_cast<const unsigned*>(P.rew) + (size_t)lead * SDC_N_AGENTS;
    const unsigned d = (mine[0] ^ his[0]) | (mine[1] ^ his[1]) | (mine[2] ^ his[2]) | (unsigned)(P.done[env] ^ P.done[lead]);
    differs = d != 0u;
  }
  const unsigned long long votes = __ballot(differs);
  const unsigned row = ((unsigned)threadIdx.x % SDC_WAVE) / SDC_MPCG_AGREE_ROW;
  const unsigned mine = (unsigned)(votes >> (row * SDC_MPCG_AGREE_ROW)) & ((1u << SDC_MPCG_AGREE_ROW) - 1u);
  // (a row with a vote is a replica's, below N: nothing else votes)
  if (u == 0 && mine != 0u) atomicAdd(P.diverged + env / R, 1);
}

hipError_t sdc_mpc_group_fold_launch(const SdcMpcGroupFold& P, hipStream_t st) {
  const size_t lanes = (size_t)(P.planned ? P.n_groups : P.n_envs) * SDC_N_AGENTS;
  const int blocks = (int)((lanes + SDC_MPCG_BLOCK - 1) / SDC_MPCG_BLOCK);
  hipLaunchKernelGGL(sdc_mpc_group_fold_kernel, dim3(blocks), dim3(SDC_MPCG_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_group_agree_launch(const SdcGroupAgree& P, hipStream_t st) {
  const size_t lanes = (size_t)((P.n_envs + 3) / 4) * SDC_WAVE;      // whole wavefronts of four envs
  const int blocks = (int)((lanes + SDC_MPCG_AGREE_BLOCK - 1) / SDC_MPCG_AGREE_BLOCK);
  hipLaunchKernelGGL(sdc_group_agree_kernel, dim3(blocks), dim3(SDC_MPCG_AGREE_BLOCK), 0, st, P);
  return hipGetLastError();
}
