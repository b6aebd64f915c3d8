// sdc_policy_stats.hpp -- what sdc_rollout_actor_stats (sdc_capi.hip) hands to sdc_policy_stats_kernel (sdc_policy_stats.hip), and the
// layout of the handle's buffer the chunk's actions and logits go into.
//
// THE KERNEL runs once per rollout chunk, behind sdc_stats_reduce_kernel, over the actions and logits sdc_rollout_actor wrote for the
// chunk, and folds them into the caller's per-(env, agent) policy statistics.  ONE LANE PER (ENV, AGENT): lane t < 3 N owns
// (n, a) = (t / 3, t % 3) -- its three action counts, its switches, LAST (5 int32) and LOGP, ENTROPY (2 doubles) stay in registers over
// the chunk's steps.  A step's actions [N][3] are a dword per lane and its logits [N][3][3] twelve contiguous bytes per lane, consecutive
// lanes on consecutive addresses: both arrays are read densely, 48 bytes per env-step.  No LDS, no barriers, no cross-lane traffic.  A
// lane's loads of different steps do not depend on each other: the step loop is unrolled by SDC_STATS_UNROLL (sdc_stats.hpp), all of a
// group's loads issued before the first is consumed; the accumulation stays in step order.  One wavefront per workgroup: there is
// nothing a workgroup shares, the time is the fp64 exp / log sequences (three exp and one log per lane and step), and 3 N lanes are few
// wavefronts -- 192 at 4096 envs -- that small workgroups spread over more CUs.
//
// EVERY ADDRESS IS BELOW ITS ARRAY'S END: with t < 3 N and k < steps a lane forms
//   actions  k * 3 N + t                <  steps * 3 N          (dwords of [steps][N][3])
//   logits   (k * 3 N + t) * 3 + 2      <  steps * 9 N          (dwords of [steps][N][3][3])
//   counts   t * 5 + 4                  <  15 N                 (dwords of [N][3][5])
//   sums     t * 2 + 1                  <  6 N                  (doubles of [N][3][2])
// and a lane t >= 3 N of the partial last wavefront loads and stores nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"

#define SDC_POLICY_BLOCK 64           // lanes per workgroup (one wavefront)
#define SDC_POLICY_WAVES_PER_EU 4     // wavefronts per SIMD the register allocation is held to, at least

// the handle's buffer for a chunk of `chunk` steps of N envs: actions [chunk][N][3] int32, then logits [chunk][N][3][3] fp32 -- 48 bytes
// per env-step.  A chunk shorter than `chunk` fills the front of each array
struct SdcPolicyBlock {      // byte offsets
  size_t actions, logits, bytes;
};
inline SdcPolicyBlock sdc_policy_block(const size_t N, const size_t chunk) {
  SdcPolicyBlock B;
  B.actions = 0;
  B.logits = chunk * N * SDC_N_AGENTS * sizeof(int32_t);
  B.bytes = B.logits + chunk * N * SDC_N_AGENTS * 3 * sizeof(float);
  return B;
}

struct SdcPolicyStats {
  int n_envs;
  int steps;                // of this chunk
  int init;                 // 1: start from N0 = N1 = N2 = SWITCHES = 0, LAST = -1, LOGP = ENTROPY = 0.0; 0: from what the arrays hold
  const int32_t* actions;   // [steps][N][3]
  const float* logits;      // [steps][N][3][3]
  int32_t* counts;          // [N][3][SDC_POLICY_COUNTS]
  double* sums;             // [N][3][SDC_POLICY_SUMS], 16-byte aligned
};

hipError_t sdc_policy_stats_launch(const SdcPolicyStats& P, hipStream_t st);
