// sdc_stats.hpp -- what sdc_rollout_stats (sdc_capi.hip) hands to sdc_stats_reduce_kernel and sdc_stats_last_kernel (sdc_stats.hip).
//
// THE REDUCE KERNEL runs once per rollout chunk over the handle's output block (sdc_plan.hpp) and folds the chunk's info and rew rows
// into the caller's per-env statistics.  FOUR ENVS PER WAVEFRONT, one row of 16 lanes per env:
//   lanes 0 .. 10 of a row   one 16-byte unit of the env's 176-byte info row each (the block's info array is 256-byte aligned and a row is
//                            eleven units, so every unit is 16-byte aligned); the four rows of a wavefront are 704 contiguous bytes per step
//   lane 11                  the env's three rew dwords and the step count
//   lanes 12 .. 15           idle
// A lane keeps the 4 fields x 4 columns of its unit in registers (16 doubles, compile-time indices only); lane 9 -- the unit of
// info[fault] -- also keeps the OR of the fault bits.  No LDS, no barriers, no cross-lane traffic.  A lane's loads of different steps do
// not depend on each other: the step loop is unrolled by SDC_STATS_UNROLL, all of a group's loads issued before the first is consumed;
// the accumulation stays in step order.  (The score kernel's shape -- one lane per env, an LDS tile filled twice per step -- is a chain of
// dependent fills, tolerable for a plan's 8 steps, not for a chunk of ~100.)
// Stores: a lane's 4 columns of a field are 32 contiguous bytes, consecutive lanes on consecutive addresses within an env and across envs.
// A partial last wavefront loads and stores nothing for its missing envs.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"

#define SDC_STATS_BLOCK 256      // reduce kernel: lanes per workgroup (four wavefronts, 16 envs)
#define SDC_STATS_ROW 16         // ... lanes per env
#define SDC_STATS_UNROLL 4       // ... steps whose loads are in flight together
#define SDC_STATS_LAST_BLOCK 256

struct SdcStatsReduce {
  int n_envs;
  int steps;               // of this chunk
  int init;                // 1: start from SUM 0, MIN +inf, MAX -inf, NPOS 0, returns 0, counts 0; 0: from what the arrays hold
  const float* rew;        // [steps][N][3]
  const float* info;       // [steps][N][44], 16-byte aligned
  double* stats;           // [SDC_STATS_FIELDS][N][44], 16-byte aligned
  double* returns;         // [N][3]
  int32_t* counts;         // [N][2]
};

// the last step's rows of the output block -> the caller's single-step arrays; final_obs in the rows of the envs that finished
struct SdcStatsLast {
  int n_envs;
  const float *obs, *share_obs, *rew, *info, *final_obs;      // the block's: the LAST step's slices, the block's final_obs
  const unsigned char* done;
  float *o_obs, *o_share_obs, *o_rew, *o_info, *o_final_obs;   // the caller's (o_rew, o_info, o_final_obs may be nullptr)
  unsigned char* o_done;                                       // (may be nullptr)
};

hipError_t sdc_stats_reduce_launch(const SdcStatsReduce& P, hipStream_t st);
hipError_t sdc_stats_last_launch(const SdcStatsLast& P, hipStream_t st);
