// sdc_mpc.hpp -- what sdc_rollout_cem_stats (sdc_capi.hip) hands to its two kernels (sdc_mpc.hip): what the Python agent
// (dc_rl_amd/agents.py CEMMPCAgent) does between two decisions, on the device.  The decision schedule -- which of the two a step
// launches, and with what -- is the host's: sdc_mpc_schedule.hpp.
//
// sdc_mpc_start_kernel, in front of a PLANNED decision of K steps, prepares the distribution and the incumbent the planner starts from:
//   fresh    probs[k] = 1.0 / 3.0 (the double), best_seq[k] = idle_action, for k < K
//   shifted  probs[k] = probs[k + 1], best_seq[k] = best_seq[k + 1] for k < K - 1, then step K - 1 as in `fresh`
// sdc_mpc_fold_kernel, behind the decision and in front of the step, folds what the planner chose into the caller's statistics and, for
// an IDLE decision, writes idle_action into best_action, so that the step reads one array either way:
//   j = the action played;  N_j += 1;  SWITCHES += (LAST >= 0 && j != LAST) ? 1 : 0;  LAST = j          (plan_counts, per env and agent)
//   planned:  SCORE += s_last;  GAIN += s_last - s_first;  PLANNED += 1.0        idle:  IDLE += 1.0       (plan_sums, per env, fp64)
//
// ONE LANE PER (ENV, AGENT) in both: lane t < 3 N owns (n, a) = (t / 3, t % 3).  A step's probs [N][3][3] are 24 contiguous bytes per
// lane, its best_seq [N][3] and best_action [N][3] a dword per lane, plan_counts [N][3][5] five dwords per lane -- consecutive lanes on
// consecutive addresses, every array read and written densely.  The lane with a == 0 also owns its env's plan_sums row (32 bytes, two
// 16-byte accesses).  No LDS, no barriers, no cross-lane traffic; one wavefront per workgroup, as sdc_policy_stats_kernel.
//
// EVERY ADDRESS IS BELOW ITS ARRAY'S END: with t < 3 N and k < K <= H (the arrays' leading dimension) a lane forms
//   probs        (k * 3 N + t) * 3 + 2   <  K * 9 N     (doubles of [K][N][3][3]; the shift reads k + 1 <= K - 1 only)
//   best_seq     k * 3 N + t             <  K * 3 N     (dwords of [K][N][3])
//   best_action  t                       <  3 N
//   plan_counts  t * 5 + 4               <  15 N
//   plan_sums    (t / 3) * 4 + 3         <  4 N         (doubles of [N][4])
//   score rows   t / 3                   <  N           (doubles of best_score's rows [N])
// and a lane t >= 3 N of the partial last wavefront loads and stores nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"

#define SDC_MPC_BLOCK 64      // lanes per workgroup (one wavefront)
#define SDC_MPC_UNROLL 4      // steps of the shift whose loads are in flight together

struct SdcMpcStart {
  int n_envs;
  int steps;            // K of this decision
  int fresh;            // 1: the fresh fill; 0: the in-place shift
  int idle[3];          // idle_action
  double* probs;        // [>= K][N][3][3]
  int32_t* best_seq;    // [>= K][N][3]
};

struct SdcMpcFold {
  int n_envs;
  int planned;               // 1: the decision was planned (best_action holds its choice); 0: idle (best_action is written)
  int init;                  // 1: start from N_j = SWITCHES = 0, LAST = -1, sums 0.0; 0: from what the arrays hold
  int idle[3];               // idle_action
  const double* score_first; // best_score[0]      [N]  (planned)
  const double* score_last;  // best_score[I - 1]  [N]  (planned)
  int32_t* best_action;      // [N][3]
  int32_t* counts;           // plan_counts [N][3][SDC_POLICY_COUNTS], or nullptr: no statistics
  double* sums;              // plan_sums [N][SDC_PLAN_SUMS], 16-byte aligned (nullptr with counts)
};

hipError_t sdc_mpc_start_launch(const SdcMpcStart& P, hipStream_t st);
hipError_t sdc_mpc_fold_launch(const SdcMpcFold& P, hipStream_t st);
