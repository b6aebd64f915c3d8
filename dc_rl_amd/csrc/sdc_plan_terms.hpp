// sdc_plan_terms.hpp -- what the plan calls (sdc_capi.hip plan_candidates) hand to sdc_plan_score_terms_kernel (sdc_plan_terms.hip)
// while plan terms are set on the handle (sdc_set_plan_terms): sdc_plan_score_kernel's plan (sdc_plan.hpp, which also describes the
// output block and the LDS tile) and, next to it, the limits and the terminal term.  All of it goes by value.
#pragma once

#include "sdc_plan.hpp"

// Up to eight info columns as a byte each, entry j in bits [8 j, 8 j + 8): two scalar registers where an int array takes eight -- the
// kernel holds the objective's, the limits' and the terminal columns next to 27 fp64 weights and bounds, and a wavefront has 102
static_assert(SDC_INFO_DIM <= 256 && SDC_PLAN_MAX_COLS <= 8 && SDC_PLAN_MAX_LIMITS <= 8 && SDC_PLAN_MAX_TERMINAL <= 8, "a byte per column");
inline uint64_t sdc_plan_pack_cols(const int32_t* col, const int n) {
  uint64_t p = 0;
  for (int j = 0; j < n; j++) p |= (uint64_t)(uint32_t)col[j] << (8 * j);
  return p;
}
__host__ __device__ inline int sdc_plan_packed_col(const uint64_t p, const int j) { return (int)((p >> (8 * j)) & 0xffu); }

struct SdcPlanScoreTerms {
  SdcPlanScore S;
  int n_steps;             // of the whole horizon: the terminal term belongs to step n_steps - 1, whichever chunk holds it
  int n_limits, n_terminal;
  double g_terminal;       // g[n_steps - 1] * gamma, multiplied on the host
  uint64_t cols, limit_cols, terminal_cols;      // a byte per entry (sdc_plan_pack_cols): S.col is not read
  uint32_t limit_upper;    // bit j: limit j is an upper bound (limit_side[j] = +1)
  double limit_bound[SDC_PLAN_MAX_LIMITS];
  double limit_weight[SDC_PLAN_MAX_LIMITS];
  double terminal_weight[SDC_PLAN_MAX_TERMINAL];
};

hipError_t sdc_plan_score_terms_launch(const SdcPlanScoreTerms& T, hipStream_t st);
