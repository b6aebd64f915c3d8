// sdc_mpc_groups.hpp -- what sdc_rollout_cem_groups_stats (sdc_capi.hip) hands to its two kernels (sdc_mpc_groups.hip): what the Python
// agent (dc_rl_amd/agents.py GroupCEMMPCAgent) does between two decisions, on the device, and the check that a group's replicas still
// agree.  The batch is G groups of R consecutive envs (N = G R).  The kernel IN FRONT of a planned decision is sdc_mpc_start_kernel
// itself (sdc_mpc.hpp) with n_envs = G: probs [K][G][3][3] and best_seq [K][G][3] have its layout.
//
// sdc_mpc_group_fold_kernel, behind the decision and in front of the step, is sdc_mpc_fold_kernel's rule per GROUP:
//   j = best_action[g][a];  N_j += 1;  SWITCHES += (LAST >= 0 && j != LAST) ? 1 : 0;  LAST = j               (plan_counts, per group and agent)
//   planned:  SCORE += s_last;  GAIN += s_last - s_first;  PLANNED += 1.0        idle:  IDLE += 1.0           (plan_sums, per group, fp64)
// and, for an IDLE decision, writes idle_action into best_action [G][3] and into every row of step_actions [N][3], so that the step reads
// one array either way (a planned decision's step_actions are the refit kernel's).  With `init` the lane of agent 0 also starts its
// group's `diverged` at 0.  ONE LANE PER DWORD of the widest array it touches: lane t < 3 G owns (g, a) = (t / 3, t % 3) -- its dword
// of best_action, five dwords of plan_counts, with a == 0 the group's plan_sums row (32 bytes, two 16-byte accesses) and dword of
// diverged --, and on an idle decision lane t < 3 N owns dword t of step_actions: consecutive lanes on consecutive addresses, every
// array read and written densely.  The launch covers 3 G lanes of a planned decision, 3 N of an idle one.  No LDS, no barriers, no
// cross-lane traffic; one wavefront per workgroup.
//
// sdc_group_agree_kernel, behind the step's reduce, compares every replica's one-step rows in the handle's output block with its group's
// first env's, bit for bit, and counts the replicas that differ.  The reduce kernel's mapping (sdc_stats.hpp): FOUR ENVS PER WAVEFRONT,
// one row of 16 lanes per env n, its leader l = n - n % R:
//   lanes 0 .. 10 of a row   one 16-byte unit of n's 176-byte info row and the same unit of l's (the block's info array is 256-byte
//                            aligned, a row is eleven units); the dword of info[reserved] is left out of the comparison
//   lane 11                  the three rew dwords and the done byte of n and of l
//   lanes 12 .. 15           idle
// A row-wide ballot of "my bits differ" decides; lane 0 of a differing row makes ONE integer atomic add on diverged[n / R].  Integer
// additions commute: the result does not depend on their order, and a batch whose replicas agree issues no atomic at all.  A group's
// first env compares nothing (n == l) and never counts.  No LDS, no barriers.
//
// EVERY ADDRESS IS BELOW ITS ARRAY'S END.  Fold, with t < 3 G (and t < 3 N where step_actions is written):
//   best_action  t                       <  3 G
//   plan_counts  t * 5 + 4               <  15 G
//   plan_sums    (t / 3) * 4 + 3         <  4 G         (doubles of [G][4])
//   score rows   t / 3                   <  G           (doubles of best_score's rows [G])
//   diverged     t / 3                   <  G
//   step_actions t                       <  3 N
// Agree, with n < N, l <= n and unit u < 11:
//   info         (n * 11 + u) * 4 + 3    <  44 N        (dwords of the step's [N][44])
//   rew          n * 3 + 2               <  3 N
//   done         n                       <  N
//   diverged     n / R                   <  G           (N = G R)
// and a lane of an env past the batch's last -- the partial last wavefront -- loads and stores nothing, as do a row's idle lanes.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"

#define SDC_MPCG_BLOCK 64         // fold kernel: lanes per workgroup (one wavefront)
#define SDC_MPCG_AGREE_BLOCK 256  // agree kernel: lanes per workgroup (four wavefronts, 16 envs)
#define SDC_MPCG_AGREE_ROW 16     // ... lanes per env

struct SdcMpcGroupFold {
  int n_envs, n_groups;
  int planned;               // 1: the decision was planned (best_action / step_actions hold its choice); 0: idle (both are written)
  int init;                  // 1: start from N_j = SWITCHES = 0, LAST = -1, sums 0.0, diverged 0; 0: from what the arrays hold
  int idle[3];               // idle_action
  const double* score_first; // best_score[0]      [G]  (planned)
  const double* score_last;  // best_score[I - 1]  [G]  (planned)
  int32_t* best_action;      // [G][3]
  int32_t* step_actions;     // [N][3]
  int32_t* counts;           // plan_counts [G][3][SDC_POLICY_COUNTS], or nullptr: no statistics
  double* sums;              // plan_sums [G][SDC_PLAN_SUMS], 16-byte aligned (nullptr with counts)
  int32_t* diverged;         // [G] (nullptr with counts)
};

struct SdcGroupAgree {
  int n_envs, group_size;
  const float* rew;           // the step's [N][3]
  const float* info;          // the step's [N][44], 16-byte aligned
  const unsigned char* done;  // the step's [N]
  int32_t* diverged;          // [G]
};

hipError_t sdc_mpc_group_fold_launch(const SdcMpcGroupFold& P, hipStream_t st);
hipError_t sdc_group_agree_launch(const SdcGroupAgree& P, hipStream_t st);
