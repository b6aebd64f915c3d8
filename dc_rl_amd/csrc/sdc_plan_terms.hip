// sdc_plan_terms.hip -- sdc_plan_score_terms_kernel: sdc_plan_score_kernel (sdc_plan.hip) with the handle's plan terms in the score:
// per step a hinge penalty on up to SDC_PLAN_MAX_LIMITS info columns, and after the horizon's last step a weighted sum of up to
// SDC_PLAN_MAX_TERMINAL columns of that step's info row (the contract and the arithmetic: include/sustaindc_hip.h sdc_set_plan_terms;
// the plan: sdc_plan_terms.hpp).  The plan calls launch it in place of sdc_plan_score_kernel while terms are set.
//
// The shape is sdc_plan_score_kernel's: one lane per env, one wavefront per workgroup, the step's info rows through the padded
// half-block LDS tile in two fills of 16-byte units; a lane picks the objective's, the limits' and -- on the horizon's last step --
// the terminal columns from its own tile row, all from the same fill (the terminal columns are weighed behind the loop).  The arithmetic is fp64 without fused multiply-adds (the
// library is built with -ffp-contract=off), the steps in order; a chunk that is not the horizon's first continues from the stored
// sums.  Every address a lane forms is below its array's end: a lane past the batch's last env loads and stores nothing, the last
// workgroup's fill stops at the batch's last info row, and the columns are in [0, SDC_INFO_DIM) (sdc_plan and sdc_set_plan_terms
// refuse others).  What decides whether a step stages its info rows, and how many columns a lane picks, is the same in every lane:
// both barriers are reached by all 64 lanes.
//
// The tile fill is a copy of sdc_plan.hip's, not a helper the two share: the resource figures of sdc_plan_score_kernel are pinned
// (tests/test_plan_abi.py), and that translation unit stays as it is.
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_plan_terms.hpp"
#include "sdc_rowcopy.hpp"

namespace {

constexpr int ROW_UNITS = SDC_INFO_DIM / 4;      // 16-byte units per info row
constexpr int TILE_DW = SDC_INFO_DIM + 1;        // a tile row: padded by a dword
static_assert(SDC_INFO_DIM % 4 == 0, "an info row is whole 16-byte units");
static_assert(SDC_PLAN_SCORE_BLOCK == SDC_WAVE && 2 * SDC_PLAN_TILE_ROWS == SDC_PLAN_SCORE_BLOCK, "one wavefront, two tile fills per step");
static_assert(SDC_PLAN_TILE_LOADS * SDC_PLAN_SCORE_BLOCK >= SDC_PLAN_TILE_ROWS * ROW_UNITS, "a fill's loads cover the half block");
static_assert(4 * SDC_PLAN_TILE_ROWS * TILE_DW <= 10240, "16 wavefronts' tiles fit a CU's LDS: four per SIMD");

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_PLAN_SCORE_BLOCK) sdc_plan_score_terms_kernel(SdcPlanScoreTerms T) {
  __shared__ float tile[SDC_PLAN_TILE_ROWS][TILE_DW];
  const int lane = (int)threadIdx.x, N = T.S.n_envs;
  const int env0 = (int)blockIdx.x * SDC_PLAN_SCORE_BLOCK, env = env0 + lane;
  const bool live = env < N;
  double ret0 = 0.0, ret1 = 0.0, ret2 = 0.0, score = 0.0;
  // the terminal columns of the lane's row, picked in the horizon's last step and weighed behind the loop: the eight weights are
  // scalar registers the loop then does not hold (the limits' bounds and weights and the objective's leave no room for them)
  float z[SDC_PLAN_MAX_TERMINAL];
#pragma unroll
  for (int j = 0; j < SDC_PLAN_MAX_TERMINAL; j++) z[j] = 0.0f;
  if (live && T.S.first_step > 0) {
    score = T.S.score[env];
    if (T.S.returns) {
      ret0 = T.S.returns[(size_t)env * 3];
      ret1 = T.S.returns[(size_t)env * 3 + 1];
      ret2 = T.S.returns[(size_t)env * 3 + 2];
    }
  }
#pragma unroll 1
  for (int k = 0; k < T.S.steps; k++) {
    const double g = T.S.g[T.S.first_step + k];
    // the terminal columns a lane picks in this step: the term's on the horizon's last step, none before (the same in every lane)
    const int n_term = T.S.first_step + k == T.n_steps - 1 ? T.n_terminal : 0;
    const size_t row0 = (size_t)k * (size_t)N;      // the step's first row
    // Whatever does not change from step to step the compiler computes in front of the loop and keeps in scalar registers: the
    // fills' lane masks, a mask per "entry j is in use", every column's offset.  Next to the 27 fp64 weights and bounds that is
    // more than the 102 a wavefront has (44 to 104 spilled as this kernel was being written).  These copies are opaque to it
    // (scalar registers in, the same out, no instruction), so what hangs on them -- a few scalar operations a step -- stays in
    // the loop.  They are the same in every lane, as the plan's fields are.
    int Nk = N, n_cols = T.S.n_cols, n_limits = T.n_limits;
    uint64_t cols = T.cols, limit_cols = T.limit_cols, terminal_cols = T.terminal_cols;
    uint32_t upper = T.limit_upper;
    asm volatile("" : "+s"(Nk), "+s"(n_cols), "+s"(n_limits), "+s"(cols), "+s"(limit_cols), "+s"(terminal_cols), "+s"(upper));
    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
    if (live) {
      const float* const r = T.S.rew + (row0 + (size_t)env) * 3;
      r0 = r[0];
      r1 = r[1];
      r2 = r[2];
    }
    double s = (T.S.w[0] * (double)r0 + T.S.w[1] * (double)r1) + T.S.w[2] * (double)r2;
    if (n_cols > 0 || n_limits > 0 || n_term > 0) {      // (the same in every lane: the barriers are inside, whole)
      float c[SDC_PLAN_MAX_COLS], x[SDC_PLAN_MAX_LIMITS];
#pragma unroll
      for (int j = 0; j < SDC_PLAN_MAX_COLS; j++) c[j] = 0.0f;
#pragma unroll
      for (int j = 0; j < SDC_PLAN_MAX_LIMITS; j++) x[j] = 0.0f;
#pragma unroll
      for (int half = 0; half < 2; half++) {
        // the half block's rows that exist, as 16-byte units: consecutive lanes on consecutive units, every load before the first store
        const int first = env0 + half * SDC_PLAN_TILE_ROWS;
        const int units = min(max(Nk - first, 0), SDC_PLAN_TILE_ROWS) * ROW_UNITS;
        const u32x4* const src = reinterpret_cast<const u32x4*>(T.S.info + (row0 + (size_t)first) * SDC_INFO_DIM);
        u32x4 v[SDC_PLAN_TILE_LOADS];
#pragma unroll
        for (int i = 0; i < SDC_PLAN_TILE_LOADS; i++) {
          const int u = lane + SDC_PLAN_SCORE_BLOCK * i;
          v[i] = u32x4{0u, 0u, 0u, 0u};
          if (u < units) v[i] = src[u];
        }
#pragma unroll
        for (int i = 0; i < SDC_PLAN_TILE_LOADS; i++) {
          const int u = lane + SDC_PLAN_SCORE_BLOCK * i;
          if ((i + 1) * SDC_PLAN_SCORE_BLOCK <= SDC_PLAN_TILE_ROWS * ROW_UNITS || u < SDC_PLAN_TILE_ROWS * ROW_UNITS) {      // (the last load's upper lanes)
            float* const q = &tile[u / ROW_UNITS][4 * (u % ROW_UNITS)];
            q[0] = __uint_as_float(v[i].x);
            q[1] = __uint_as_float(v[i].y);
            q[2] = __uint_as_float(v[i].z);
            q[3] = __uint_as_float(v[i].w);
          }
        }
        __syncthreads();
        if ((lane >> 5) == half) {
          const float* const mine = tile[lane & (SDC_PLAN_TILE_ROWS - 1)];
          // (constant indices into the by-value plan: no copy of it in scratch memory)
#pragma unroll
          for (int j = 0; j < SDC_PLAN_MAX_COLS; j++)
            if (j < n_cols) c[j] = mine[sdc_plan_packed_col(cols, j)];
#pragma unroll
          for (int j = 0; j < SDC_PLAN_MAX_LIMITS; j++)
            if (j < n_limits) x[j] = mine[sdc_plan_packed_col(limit_cols, j)];
#pragma unroll
          for (int j = 0; j < SDC_PLAN_MAX_TERMINAL; j++)
            if (j < n_term) z[j] = mine[sdc_plan_packed_col(terminal_cols, j)];
        }
        __syncthreads();
      }
#pragma unroll
      for (int j = 0; j < SDC_PLAN_MAX_COLS; j++)
        if (j < n_cols) s += T.S.col_weight[j] * (double)c[j];
#pragma unroll
      for (int j = 0; j < SDC_PLAN_MAX_LIMITS; j++)
        if (j < n_limits) {
          const double d = ((upper >> j) & 1u) != 0u ? (double)x[j] - T.limit_bound[j] : T.limit_bound[j] - (double)x[j];
          const double e = d > 0.0 ? d : 0.0;
          s = s - T.limit_weight[j] * e;
        }
    }
    ret0 += g * (double)r0;
    ret1 += g * (double)r1;
    ret2 += g * (double)r2;
    score += g * s;
  }
  // behind the horizon's last step, which is the last of the chunk that holds it (the same in every lane)
  if (T.S.first_step + T.S.steps == T.n_steps && T.n_terminal > 0) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < SDC_PLAN_MAX_TERMINAL; j++)
      if (j < T.n_terminal) t += T.terminal_weight[j] * (double)z[j];
    score += T.g_terminal * t;
  }
  if (live) {
    T.S.score[env] = score;
    if (T.S.returns) {
      T.S.returns[(size_t)env * 3] = ret0;
      T.S.returns[(size_t)env * 3 + 1] = ret1;
      T.S.returns[(size_t)env * 3 + 2] = ret2;
    }
  }
}

hipError_t sdc_plan_score_terms_launch(const SdcPlanScoreTerms& T, hipStream_t st) {
  const int blocks = (T.S.n_envs + SDC_PLAN_SCORE_BLOCK - 1) / SDC_PLAN_SCORE_BLOCK;
  hipLaunchKernelGGL(sdc_plan_score_terms_kernel, dim3(blocks), dim3(SDC_PLAN_SCORE_BLOCK), 0, st, T);
  return hipGetLastError();
}
