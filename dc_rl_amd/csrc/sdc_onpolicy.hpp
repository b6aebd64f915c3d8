// sdc_onpolicy.hpp -- what sdc_gae and sdc_action_log_probs (sdc_capi.hip) hand to the three kernels of sdc_onpolicy.hip: the part of an
// on-policy training batch that is neither the rollout's nor the critic's -- returns, advantages, masks, normalised value predictions
// and the advantages' moments (the reference's OnPolicyCriticBufferEP.compute_returns and what its runners do around it), and the
// log-probability of every action played.  The arithmetic: include/sustaindc_hip.h THE ON-POLICY BATCH.
//
// sdc_gae_kernel: ONE LANE PER ENV, one wavefront per workgroup (nothing is shared between envs, and N / 64 wavefronts are few -- 64 at
// 4096 envs -- that small workgroups spread over more CUs: sdc_policy_stats.hpp).  The lane walks t = T-1 .. 0 with gae (or the running
// return) and V[t+1] in registers.  Per step it loads
//   done   one byte:            a wavefront's 64 lanes read 64 consecutive bytes of row t of [T][N], one or two 64-byte lines
//   rew    one dword:           column reward_agent of its env's three, 12 bytes from lane to lane -- the wavefront's loads fall into the
//                               768 contiguous bytes of its 64 envs' rows of [T][N][3], six or seven 128-byte lines that are fetched once
//                               whichever way they are read; a lane that loaded all three dwords to choose one in registers would
//                               fetch the same lines and hold two registers more per step in flight
//   V[t]   one dword, dense
// and stores one dense dword each of returns, advantages, masks and (optional) value_preds.  None of a step's loads depends on the
// recurrence: the step loop is unrolled by SDC_STATS_UNROLL (sdc_stats.hpp), all of a group's loads issued before the first is
// consumed; only the chain of three operations per step (use_gae: multiply, add into delta's partner, add) is serial.  A
// parallel-in-time scan would re-associate the recurrence and change its rounding; bit-equality with the reference's order is the
// point.  No LDS, no barriers, no cross-lane traffic, no atomics.
//
// EVERY ADDRESS IS BELOW ITS ARRAY'S END: with n < N and 0 <= t < T a lane forms
//   rew          (t * N + n) * 3 + a      <  3 T N         (dwords of [T][N][3]; a = reward_agent <= 2, held to 0 .. 2 by sdc_gae)
//   done         t * N + n                <  T N           (bytes of [T][N])
//   first_done   n                        <  N             (bytes of [N])
//   values       (t + 1) * N + n          <  (T + 1) N     (dwords of [T+1][N]; row T is the first load)
//   returns, advantages   t * N + n       <  T N           (dwords of [T][N])
//   masks, value_preds    (t + 1) * N + n <  (T + 1) N     (dwords of [T+1][N]; row 0 is written behind the walk)
//   adv_part     n * 2 + 1                <  2 N           (doubles of [N][2])
// and a lane n >= N of the partial last wavefront loads and stores nothing.
//
// sdc_adv_moments_kernel: ONE workgroup of SDC_MOMENTS_BLOCK lanes folds adv_part [N][2] into moments[2].  Lane l adds the pairs of envs
// l, l + B, l + 2 B, ... in that order, then the B partial pairs are halved log2(B) times through LDS (entry i += entry i + half): the
// order is fixed by N alone.  adv_part index (l + k B) * 2 + 1 < 2 N by the loop's bound.
//
// sdc_action_logp_kernel: elementwise, ONE LANE PER (STEP, ENV, AGENT) in grid-stride: element i < 3 T N loads dword i of actions and
// dwords 3 i .. 3 i + 2 of logits (< 9 T N) -- both dense across a wavefront -- and stores dword i of log_probs and of entropy.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"
#include "sdc_critic_pack.hpp"

#define SDC_GAE_BLOCK 64           // lanes per workgroup (one wavefront)
#define SDC_MOMENTS_BLOCK 256      // the single workgroup of the moments kernel (a power of two)
#define SDC_LOGP_BLOCK 256
#define SDC_LOGP_MAX_BLOCKS 2048   // ... of 256 CUs, eight workgroups each; more elements: more passes of the grid

struct SdcGae {
  int n_envs;
  int steps;                   // T
  int reward_agent;            // the column of rew, 0 .. 2
  int use_gae;
  float g, c;                  // (float)gamma, (float)(gamma * gae_lambda)
  const float* rew;            // [T][N][3]
  const uint8_t* done;         // [T][N]
  const uint8_t* first_done;   // [N] or nullptr (masks[0] = 1)
  const float* values;         // [T+1][N]
  float* returns;              // [T][N]
  float* advantages;           // [T][N]
  float* masks;                // [T+1][N]
  float* value_preds;          // [T+1][N] or nullptr
  const SdcCriticDev* critic;  // its scale and shift: read only when value_preds is given
  double* adv_part;            // [N][2], 16-byte aligned
};

struct SdcAdvMoments {
  int n_envs;
  double count;                // T * N
  const double* adv_part;      // [N][2]
  double* moments;             // [2]: mean, population standard deviation
};

struct SdcActionLogp {
  long long n;                 // 3 T N
  const int32_t* actions;      // [T][N][3]
  const float* logits;         // [T][N][3][3]
  float* log_probs;            // [T][N][3]
  float* entropy;              // [T][N][3] or nullptr
};

hipError_t sdc_gae_launch(const SdcGae& P, hipStream_t st);
hipError_t sdc_adv_moments_launch(const SdcAdvMoments& P, hipStream_t st);
hipError_t sdc_action_logp_launch(const SdcActionLogp& P, hipStream_t st);
