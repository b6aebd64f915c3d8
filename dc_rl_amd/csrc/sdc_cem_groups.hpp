// sdc_cem_groups.hpp -- what sdc_plan_cem_groups (sdc_capi.hip) hands to sdc_cem_group_sample_kernel and sdc_cem_group_refit_kernel
// (sdc_cem_groups.hip): the cross-entropy method with the candidates in env slots.  The batch is G groups of R consecutive envs
// (replicas) that hold one state; replica r of group g plays the role candidate r of env g plays in sdc_plan_cem.  The arrays' layouts
// and the arithmetic, operation by operation: include/sustaindc_hip.h (sdc_plan_cem_groups); how the kernels move their rows and
// what they hold in LDS: sdc_cem_groups.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"

#define SDC_CEMG_SAMPLE_BLOCK 64      // sample kernel: envs (lanes) per workgroup, one wavefront
#define SDC_CEMG_SAMPLE_GROUPS 33     // ... and the most groups 64 consecutive envs can touch (R >= 2: 63 / 2 + 2)
#define SDC_CEMG_REFIT_WAVES 16       // refit kernel: wavefronts of a group's workgroup
#define SDC_CEMG_REFIT_BLOCK (64 * SDC_CEMG_REFIT_WAVES)
#define SDC_CEMG_RANK_PER_THREAD (SDC_CEM_MAX_GROUP / SDC_CEMG_REFIT_BLOCK)          // replicas a thread ranks: t, t + T, ...
#define SDC_CEMG_ROW_PER_THREAD (3 * SDC_CEM_MAX_GROUP / SDC_CEMG_REFIT_BLOCK)       // dwords of a step's cand rows a thread holds

struct SdcCemGroupSample {
  int n_envs, group_size, n_groups, n_steps;
  int group_base;            // global index of group 0 (sdc_cem_group_params.group_base)
  int fixed[3];              // per agent: -1 sampled, 0..2 the value every sampled replica carries
  unsigned draw, c3;         // counter words 2 and 3: the caller's decision counter, (it << 16) | SDC_CEM_STREAM
  unsigned key0, key1;       // seed, low and high word
  const double* probs;       // [K][G][3][3]
  const int32_t* best_seq;   // [K][G][3]
  int32_t* cand;             // [K][N][3]
};

struct SdcCemGroupRefit {
  int n_envs, group_size, n_groups, n_steps, n_elite;
  int fixed[3];
  int last;                  // the call's last iteration: best_action and step_actions are written
  double alpha, take, p_min; // take = 1.0 - alpha (the host's subtraction)
  const double* score;       // [N]
  const int32_t* cand;       // [K][N][3]
  double* probs;             // [K][G][3][3]
  int32_t* best_seq;         // [K][G][3]
  double* best_score;        // [G] this iteration's row
  int32_t* best_action;      // [G][3]
  int32_t* step_actions;     // [N][3]
};

hipError_t sdc_cem_group_sample_launch(const SdcCemGroupSample& P, hipStream_t st);
hipError_t sdc_cem_group_refit_launch(const SdcCemGroupRefit& P, hipStream_t st);
