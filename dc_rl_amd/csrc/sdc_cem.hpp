// sdc_cem.hpp -- what sdc_plan_cem (sdc_capi.hip) hands to sdc_cem_sample_kernel and sdc_cem_refit_kernel (sdc_cem.hip): the
// cross-entropy method's two steps around sdc_plan's per-candidate loop.  The arrays' layouts and the arithmetic, operation by
// operation: include/sustaindc_hip.h (sdc_plan_cem); how the kernels move their rows and what they hold in LDS: sdc_cem.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"

#define SDC_CEM_SAMPLE_BLOCK 64      // sample kernel: envs (lanes) per workgroup, one wavefront
#define SDC_CEM_REFIT_ENVS 64        // refit kernel: envs per workgroup ...
#define SDC_CEM_REFIT_WAVES 4        // ... on this many wavefronts, which share the candidates (ranking) and the steps (refit)
#define SDC_CEM_STREAM 0xCE3Du       // the low half of the generator's fourth counter word

struct SdcCemSample {
  int n_envs, n_cand, n_steps;
  int env_base;              // global index of env 0 (sdc_config.env_index_base)
  int fixed[3];              // per agent: -1 sampled, 0..2 the value every sampled candidate carries
  unsigned draw, c3;         // counter words 2 and 3: the caller's decision counter, (it << 16) | SDC_CEM_STREAM
  unsigned key0, key1;       // seed, low and high word
  const double* probs;       // [K][N][3][3]
  const int32_t* best_seq;   // [K][N][3]
  int32_t* cand;             // [M][K][N][3]
};

struct SdcCemRefit {
  int n_envs, n_cand, n_steps, n_elite;
  int fixed[3];
  int last;                  // the call's last iteration: best_action is written
  double alpha, take, p_min; // take = 1.0 - alpha (the host's subtraction)
  const double* score;       // [M][N]
  const int32_t* cand;       // [M][K][N][3]
  double* probs;             // [K][N][3][3]
  int32_t* best_seq;         // [K][N][3]
  double* best_score;        // [N] this iteration's row
  int32_t* best_action;      // [N][3]
};

hipError_t sdc_cem_sample_launch(const SdcCemSample& P, hipStream_t st);
hipError_t sdc_cem_refit_launch(const SdcCemRefit& P, hipStream_t st);
