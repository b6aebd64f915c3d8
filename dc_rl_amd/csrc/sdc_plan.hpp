// sdc_plan.hpp -- what sdc_plan (sdc_capi.hip) hands to sdc_plan_score_kernel and sdc_plan_select_kernel (sdc_plan.hip), and the layout
// of the output block its rollouts write into.
//
// THE OUTPUT BLOCK belongs to the handle: the arrays sdc_rollout fills for `steps` steps, each on a 256-byte boundary (the lane-per-env
// step kernel stores whole lines: sdc_dispatch.hpp sdc_wide_structural), in this order:
//   obs [steps][N][3][26] | share_obs [steps][N][29] | rew [steps][N][3] | info [steps][N][44] | done [steps][N] | final_obs [N][3][26]
// 617 bytes per env-step, of which the score kernel reads the 12 of rew and, with info columns in the objective, the 176 of info.  The
// block is capped at SDC_PLAN_SCRATCH_BYTES; a horizon that does not fit is rolled out in chunks of sdc_plan_steps_fit steps.
//
// THE SCORE KERNEL runs once per rollout (per chunk): one LANE per env, one wavefront per workgroup, a loop over the chunk's steps.  A
// step's rew rows of 64 consecutive envs are 768 contiguous bytes.  Its info rows are 64 x 176 = 11 264 contiguous bytes of which a lane
// wants n_cols dwords of its own row: read as a dword per lane that is one 176-byte stride per lane and column (what the rewind's range
// M loses its time on), so the block comes in as whole 16-byte units, consecutive lanes on consecutive units, goes
// through LDS, and the lanes pick their columns there.  The tile holds HALF the workgroup's rows (32 rows of 45 dwords: padded by a
// dword, so the column reads of 32 lanes hit 32 banks) and is filled twice per step: a whole-block tile (11 520 bytes a wavefront) would
// leave 14 wavefronts per CU, below four per SIMD.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"

#define SDC_PLAN_SCRATCH_BYTES ((size_t)256 << 20)   // cap of the output block
#define SDC_PLAN_SCORE_BLOCK 64                      // score kernel: envs (lanes) per workgroup
#define SDC_PLAN_TILE_ROWS 32                        // ... info rows per LDS tile fill (half the workgroup's)
#define SDC_PLAN_TILE_LOADS 6                        // ... 16-byte units a lane loads per fill: ceil(32 * 11 / 64)
#define SDC_PLAN_SELECT_BLOCK 256

struct SdcPlanBlock {      // byte offsets into the output block
  size_t obs, share_obs, rew, info, done, final_obs, bytes;
};

// the block's layout for `steps` steps of N envs
inline SdcPlanBlock sdc_plan_block(const size_t N, const size_t steps) {
  const auto up = [](const size_t x) { return (x + 255u) / 256u * 256u; };
  SdcPlanBlock B;
  B.obs = 0;
  B.share_obs = up(B.obs + steps * N * sizeof(float) * SDC_N_AGENTS * SDC_OBS_PAD);
  B.rew = up(B.share_obs + steps * N * sizeof(float) * SDC_SHARE_OBS_DIM);
  B.info = up(B.rew + steps * N * sizeof(float) * SDC_N_AGENTS);
  B.done = up(B.info + steps * N * sizeof(float) * SDC_INFO_DIM);
  B.final_obs = up(B.done + steps * N);
  B.bytes = up(B.final_obs + N * sizeof(float) * SDC_N_AGENTS * SDC_OBS_PAD);
  return B;
}

// the steps of a K-step horizon a block of at most `cap` bytes holds: at least one (a batch whose single step is larger than the cap
// gets a block of one step)
inline int sdc_plan_steps_fit(const size_t N, const int K, const size_t cap) {
  int s = K;
  while (s > 1 && sdc_plan_block(N, (size_t)s).bytes > cap) s -= 1;
  return s;
}

struct SdcPlanScore {
  int n_envs;
  int steps;               // of this chunk
  int first_step;          // the chunk's first step within the horizon: its discount is g[first_step]
  int n_cols;
  const double* g;         // [n_steps] the discount table (device)
  const float* rew;        // [steps][N][3]
  const float* info;       // [steps][N][44], 16-byte aligned
  double* returns;         // [N][3] this candidate's, or nullptr
  double* score;           // [N]
  double w[3];
  double col_weight[SDC_PLAN_MAX_COLS];
  int col[SDC_PLAN_MAX_COLS];
};

struct SdcPlanSelect {
  int n_envs, n_cand, n_steps;
  const double* score;     // [M][N]
  const int32_t* actions;  // [M][K][N][3]
  int32_t* best;           // [N]
  int32_t* best_action;    // [N][3]
};

hipError_t sdc_plan_score_launch(const SdcPlanScore& P, hipStream_t st);
hipError_t sdc_plan_select_launch(const SdcPlanSelect& P, hipStream_t st);
