// sdc_plan.hip -- sdc_plan_score_kernel: a rollout's rewards and info columns -> the candidate's discounted returns and score;
// sdc_plan_select_kernel: the candidates' scores -> every env's best candidate and its first action (sdc_plan, sdc_capi.hip; the plans,
// the output block and why the info rows go through LDS: sdc_plan.hpp).
//
// The arithmetic is the one include/sustaindc_hip.h states for sdc_plan, operation by operation: fp64, no fused multiply-adds (the
// library is built with -ffp-contract=off), the steps in order.  A chunk that is not the horizon's first continues from the sums the
// chunk before it stored.  Every address a lane forms is below its array's end: a lane past the batch's last env loads and stores
// nothing, and the last workgroup's tile fill stops at the batch's last info row.
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_plan.hpp"
#include "sdc_rowcopy.hpp"

namespace {

constexpr int ROW_UNITS = SDC_INFO_DIM / 4;      // 16-byte units per info row
constexpr int TILE_DW = SDC_INFO_DIM + 1;        // a tile row: padded by a dword
static_assert(SDC_INFO_DIM % 4 == 0, "an info row is whole 16-byte units");
static_assert(SDC_PLAN_SCORE_BLOCK == SDC_WAVE && 2 * SDC_PLAN_TILE_ROWS == SDC_PLAN_SCORE_BLOCK, "one wavefront, two tile fills per step");
static_assert(SDC_PLAN_TILE_LOADS * SDC_PLAN_SCORE_BLOCK >= SDC_PLAN_TILE_ROWS * ROW_UNITS, "a fill's loads cover the half block");
static_assert(4 * SDC_PLAN_TILE_ROWS * TILE_DW <= 10240, "16 wavefronts' tiles fit a CU's LDS: four per SIMD");

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_PLAN_SCORE_BLOCK) sdc_plan_score_kernel(SdcPlanScore P) {
  __shared__ float tile[SDC_PLAN_TILE_ROWS][TILE_DW];
  const int lane = (int)threadIdx.x, N = P.n_envs;
  const int env0 = (int)blockIdx.x * SDC_PLAN_SCORE_BLOCK, env = env0 + lane;
  const bool live = env < N;
  double ret0 = 0.0, ret1 = 0.0, ret2 = 0.0, score = 0.0;
  if (live && P.first_step > 0) {
    score = P.score[env];
    if (P.returns) {
      ret0 = P.returns[(size_t)env * 3];
      ret1 = P.returns[(size_t)env * 3 + 1];
      ret2 = P.returns[(size_t)env * 3 + 2];
    }
  }
#pragma unroll 1
  for (int k = 0; k < P.steps; k++) {
    const double g = P.g[P.first_step + k];
    const size_t row0 = (size_t)k * (size_t)N;      // the step's first row
    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
    if (live) {
      const float* const r = P.rew + (row0 + (size_t)env) * 3;
      r0 = r[0];
      r1 = r[1];
      r2 = r[2];
    }
    double s = (P.w[0] * (double)r0 + P.w[1] * (double)r1) + P.w[2] * (double)r2;
    if (P.n_cols > 0) {      // (the same in every lane)
      float c[SDC_PLAN_MAX_COLS];
#pragma unroll
      for (int j = 0; j < SDC_PLAN_MAX_COLS; j++) c[j] = 0.0f;
#pragma unroll
      for (int half = 0; half < 2; half++) {
        // the half block's rows that exist, as 16-byte units: consecutive lanes on consecutive units, every load before the first store
        const int first = env0 + half * SDC_PLAN_TILE_ROWS;
        const int units = min(max(N - first, 0), SDC_PLAN_TILE_ROWS) * ROW_UNITS;
        const u32x4* const src = reinterpret_cast<const u32x4*>(P.info + (row0 + (size_t)first) * SDC_INFO_DIM);
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
          if (u < SDC_PLAN_TILE_ROWS * ROW_UNITS) {
            float* const t = &tile[u / ROW_UNITS][4 * (u % ROW_UNITS)];
            t[0] = __uint_as_float(v[i].x);
            t[1] = __uint_as_float(v[i].y);
            t[2] = __uint_as_float(v[i].z);
            t[3] = __uint_as_float(v[i].w);
          }
        }
        __syncthreads();
        if ((lane >> 5) == half) {
          const float* const mine = tile[lane & (SDC_PLAN_TILE_ROWS - 1)];
#pragma unroll
          for (int j = 0; j < SDC_PLAN_MAX_COLS; j++)      // (constant indices into the by-value plan: no copy of it in scratch memory)
            if (j < P.n_cols) c[j] = mine[P.col[j]];
        }
        __syncthreads();
      }
#pragma unroll
      for (int j = 0; j < SDC_PLAN_MAX_COLS; j++)
        if (j < P.n_cols) s += P.col_weight[j] * (double)c[j];
    }
    ret0 += g * (double)r0;
    ret1 += g * (double)r1;
    ret2 += g * (double)r2;
    score += g * s;
  }
  if (live) {
    P.score[env] = score;
    if (P.returns) {
      P.returns[(size_t)env * 3] = ret0;
      P.returns[(size_t)env * 3 + 1] = ret1;
      P.returns[(size_t)env * 3 + 2] = ret2;
    }
  }
}

// one lane per env: candidate 0, unless a later one's score is strictly greater than every earlier one's
extern "C" __global__ void __launch_bounds__(SDC_PLAN_SELECT_BLOCK) sdc_plan_select_kernel(SdcPlanSelect P) {
  const int env = (int)blockIdx.x * SDC_PLAN_SELECT_BLOCK + (int)threadIdx.x, N = P.n_envs;
  if (env >= N) return;
  double top = P.score[env];
  int best = 0;
#pragma unroll 4
  for (int c = 1; c < P.n_cand; c++) {
    const double x = P.score[(size_t)c * (size_t)N + (size_t)env];
    if (x > top) {
      top = x;
      best = c;
    }
  }
  const int32_t* const a = P.actions + ((size_t)best * (size_t)P.n_steps * (size_t)N + (size_t)env) * 3;
  const int32_t a0 = a[0], a1 = a[1], a2 = a[2];
  P.best[env] = best;
  int32_t* const o = P.best_action + (size_t)env * 3;
  o[0] = a0;
  o[1] = a1;
  o[2] = a2;
}

hipError_t sdc_plan_score_launch(const SdcPlanScore& P, hipStream_t st) {
  const int blocks = (P.n_envs + SDC_PLAN_SCORE_BLOCK - 1) / SDC_PLAN_SCORE_BLOCK;
  hipLaunchKernelGGL(sdc_plan_score_kernel, dim3(blocks), dim3(SDC_PLAN_SCORE_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_plan_select_launch(const SdcPlanSelect& P, hipStream_t st) {
  const int blocks = (P.n_envs + SDC_PLAN_SELECT_BLOCK - 1) / SDC_PLAN_SELECT_BLOCK;
  hipLaunchKernelGGL(sdc_plan_select_kernel, dim3(blocks), dim3(SDC_PLAN_SELECT_BLOCK), 0, st, P);
  return hipGetLastError();
}
