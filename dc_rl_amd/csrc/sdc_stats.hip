// sdc_stats.hip -- sdc_stats_reduce_kernel: a rollout chunk's info and rew rows -> per-env episode statistics (sum, min, max, count of
// positive values of all 44 info columns; the three agents' returns; steps; the OR of the fault bits); sdc_stats_last_kernel: the last
// step's rows of the output block -> the caller's single-step arrays (sdc_rollout_stats, sdc_capi.hip; the plans and the lane mapping:
// sdc_stats.hpp).
//
// The arithmetic is the one include/sustaindc_hip.h states for sdc_rollout_stats, operation by operation: fp64, no fused multiply-adds
// (the library is built with -ffp-contract=off), the steps in order, comparisons and selects -- not min / max instructions, whose NaN and
// signed-zero rules differ.  A chunk that is not the call's first continues from what the chunk before it stored.  Every address a lane
// forms is below its array's end: a lane of an env past the batch's last loads and stores nothing, and so do a row's idle lanes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sdc_device.hpp"
#include "sdc_rowcopy.hpp"
#include "sdc_stats.hpp"

namespace {

constexpr int ROW_UNITS = SDC_INFO_DIM / 4;      // 16-byte units per info row
constexpr int REW_LANE = ROW_UNITS;              // the lane of a row that takes rew and the step count
constexpr int FAULT_UNIT = SDC_INFO_FAULT / 4;   // the lane that owns info[fault] ...
constexpr int FAULT_DWORD = SDC_INFO_FAULT % 4;  // ... and the column's place in its unit
static_assert(SDC_INFO_DIM % 4 == 0 && ROW_UNITS < SDC_STATS_ROW, "an info row is whole 16-byte units, and a row of lanes has one to spare");
static_assert(SDC_WAVE % SDC_STATS_ROW == 0 && SDC_STATS_BLOCK % SDC_WAVE == 0, "whole rows per wavefront, whole wavefronts per workgroup");
static_assert(SDC_STATS_FIELDS == 4 && SDC_STAT_SUM == 0 && SDC_STAT_MIN == 1 && SDC_STAT_MAX == 2 && SDC_STAT_NPOS == 3, "the fields");
static_assert(FAULT_DWORD == 1, "fold_fault reads the unit's second dword");

typedef double f64x2 __attribute__((ext_vector_type(2)));

// a lane's 4 fields x 4 columns
struct Acc {
  double sum[4], lo[4], hi[4], npos[4];
  unsigned fault;
};

__device__ __forceinline__ void fold(Acc& A, const u32x4 v, const bool owns_fault) {
  const float f[4] = {__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const double x = (double)f[c];
    A.sum[c] += x;
    A.lo[c] = x < A.lo[c] ? x : A.lo[c];
    A.hi[c] = x > A.hi[c] ? x : A.hi[c];
    A.npos[c] += (x > 0.0) ? 1.0 : 0.0;
  }
  A.fault |= owns_fault ? (unsigned)f[FAULT_DWORD] : 0u;
}

// STEPS consecutive steps' 16 bytes of this lane: info units, or the env's three rew dwords (and a zero), or nothing.  One branch
// around all the loads of a class, so they are in flight together
template <int STEPS>
__device__ __forceinline__ void take(u32x4 (&v)[STEPS], const bool is_info, const bool is_rew, const u32x4* const ip, const size_t istep,
                                     const float* const rp, const size_t rstep) {
#pragma unroll
  for (int i = 0; i < STEPS; i++) v[i] = u32x4{0u, 0u, 0u, 0u};
  if (is_info) {
#pragma unroll
    for (int i = 0; i < STEPS; i++) v[i] = ip[(size_t)i * istep];
  } else if (is_rew) {
#pragma unroll
    for (int i = 0; i < STEPS; i++) {
      const float* const r = rp + (size_t)i * rstep;
      v[i].x = __float_as_uint(r[0]);
      v[i].y = __float_as_uint(r[1]);
      v[i].z = __float_as_uint(r[2]);
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_STATS_BLOCK) sdc_stats_reduce_kernel(SdcStatsReduce P) {
  const int N = P.n_envs;
  const int t = (int)blockIdx.x * SDC_STATS_BLOCK + (int)threadIdx.x;
  const int env = t / SDC_STATS_ROW, u = t % SDC_STATS_ROW;
  const bool live = env < N;
  const bool is_info = live && u < ROW_UNITS, is_rew = live && u == REW_LANE;
  const bool owns_fault = is_info && u == FAULT_UNIT;
  const size_t e = live ? (size_t)env : 0;
  // this lane's addresses at step 0, and what a step adds
  const u32x4* ip = reinterpret_cast<const u32x4*>(P.info) + e * ROW_UNITS + (size_t)(is_info ? u : 0);
  const float* rp = P.rew + e * 3;
  const size_t istep = (size_t)N * ROW_UNITS, rstep = (size_t)N * 3;
  double* const mine = P.stats + e * SDC_INFO_DIM + (size_t)(is_info ? 4 * u : 0);      // field f: + f * N * 44
  const size_t fstep = (size_t)N * SDC_INFO_DIM;

  Acc A;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    A.sum[c] = 0.0;
    A.lo[c] = __longlong_as_double(0x7ff0000000000000ll);
    A.hi[c] = __longlong_as_double((long long)0xfff0000000000000ull);
    A.npos[c] = 0.0;
  }
  A.fault = 0u;
  int count = 0;
  if (!P.init) {
    if (is_info) {
      const f64x2 s0 = *reinterpret_cast<const f64x2*>(mine), s1 = *reinterpret_cast<const f64x2*>(mine + 2);
      const f64x2 l0 = *reinterpret_cast<const f64x2*>(mine + fstep), l1 = *reinterpret_cast<const f64x2*>(mine + fstep + 2);
      const f64x2 h0 = *reinterpret_cast<const f64x2*>(mine + 2 * fstep), h1 = *reinterpret_cast<const f64x2*>(mine + 2 * fstep + 2);
      const f64x2 n0 = *reinterpret_cast<const f64x2*>(mine + 3 * fstep), n1 = *reinterpret_cast<const f64x2*>(mine + 3 * fstep + 2);
      A.sum[0] = s0.x; A.sum[1] = s0.y; A.sum[2] = s1.x; A.sum[3] = s1.y;
      A.lo[0] = l0.x; A.lo[1] = l0.y; A.lo[2] = l1.x; A.lo[3] = l1.y;
      A.hi[0] = h0.x; A.hi[1] = h0.y; A.hi[2] = h1.x; A.hi[3] = h1.y;
      A.npos[0] = n0.x; A.npos[1] = n0.y; A.npos[2] = n1.x; A.npos[3] = n1.y;
      if (owns_fault) A.fault = (unsigned)P.counts[e * 2 + 1];
    } else if (is_rew) {
      A.sum[0] = P.returns[e * 3];
      A.sum[1] = P.returns[e * 3 + 1];
      A.sum[2] = P.returns[e * 3 + 2];
      count = P.counts[e * 2];
    }
  }

  int k = 0;
#pragma unroll 1
  for (; k + SDC_STATS_UNROLL <= P.steps; k += SDC_STATS_UNROLL) {
    u32x4 v[SDC_STATS_UNROLL];
    take(v, is_info, is_rew, ip, istep, rp, rstep);
#pragma unroll
    for (int i = 0; i < SDC_STATS_UNROLL; i++) fold(A, v[i], owns_fault);
    ip += (size_t)SDC_STATS_UNROLL * istep;
    rp += (size_t)SDC_STATS_UNROLL * rstep;
  }
#pragma unroll 1
  for (; k < P.steps; k++) {
    u32x4 v[1];
    take(v, is_info, is_rew, ip, istep, rp, rstep);
    fold(A, v[0], owns_fault);
    ip += istep;
    rp += rstep;
  }

  if (is_info) {
    *reinterpret_cast<f64x2*>(mine) = f64x2{A.sum[0], A.sum[1]};
    *reinterpret_cast<f64x2*>(mine + 2) = f64x2{A.sum[2], A.sum[3]};
    *reinterpret_cast<f64x2*>(mine + fstep) = f64x2{A.lo[0], A.lo[1]};
    *reinterpret_cast<f64x2*>(mine + fstep + 2) = f64x2{A.lo[2], A.lo[3]};
    *reinterpret_cast<f64x2*>(mine + 2 * fstep) = f64x2{A.hi[0], A.hi[1]};
    *reinterpret_cast<f64x2*>(mine + 2 * fstep + 2) = f64x2{A.hi[2], A.hi[3]};
    *reinterpret_cast<f64x2*>(mine + 3 * fstep) = f64x2{A.npos[0], A.npos[1]};
    *reinterpret_cast<f64x2*>(mine + 3 * fstep + 2) = f64x2{A.npos[2], A.npos[3]};
    if (owns_fault) P.counts[e * 2 + 1] = (int32_t)A.fault;
  } else if (is_rew) {
    P.returns[e * 3] = A.sum[0];
    P.returns[e * 3 + 1] = A.sum[1];
    P.returns[e * 3 + 2] = A.sum[2];
    P.counts[e * 2] = count + P.steps;
  }
}

// a dword per lane and turn, consecutive lanes on consecutive dwords; final_obs only in the rows of the envs whose last step was terminal
// (the others keep what the caller's array held, as after sdc_rollout)
extern "C" __global__ void __launch_bounds__(SDC_STATS_LAST_BLOCK) sdc_stats_last_kernel(SdcStatsLast P) {
  const size_t N = (size_t)P.n_envs;
  const size_t stride = (size_t)gridDim.x * SDC_STATS_LAST_BLOCK;
  const size_t t0 = (size_t)blockIdx.x * SDC_STATS_LAST_BLOCK + threadIdx.x;
  for (size_t i = t0; i < N * SDC_OBS_OUT; i += stride) P.o_obs[i] = P.obs[i];
  for (size_t i = t0; i < N * SDC_SHARE_OBS_DIM; i += stride) P.o_share_obs[i] = P.share_obs[i];
  if (P.o_rew)
    for (size_t i = t0; i < N * SDC_N_AGENTS; i += stride) P.o_rew[i] = P.rew[i];
  if (P.o_info)
    for (size_t i = t0; i < N * SDC_INFO_DIM; i += stride) P.o_info[i] = P.info[i];
  if (P.o_done)
    for (size_t i = t0; i < N; i += stride) P.o_done[i] = P.done[i];
  if (P.o_final_obs)
    for (size_t i = t0; i < N * SDC_OBS_OUT; i += stride)
      if (P.done[i / SDC_OBS_OUT]) P.o_final_obs[i] = P.final_obs[i];
}

hipError_t sdc_stats_reduce_launch(const SdcStatsReduce& P, hipStream_t st) {
  const size_t lanes = (size_t)((P.n_envs + 3) / 4) * SDC_WAVE;      // whole wavefronts of four envs
  const int blocks = (int)((lanes + SDC_STATS_BLOCK - 1) / SDC_STATS_BLOCK);
  hipLaunchKernelGGL(sdc_stats_reduce_kernel, dim3(blocks), dim3(SDC_STATS_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_stats_last_launch(const SdcStatsLast& P, hipStream_t st) {
  const size_t dwords = (size_t)P.n_envs * SDC_OBS_OUT;
  const int blocks = (int)std::min<size_t>((dwords + SDC_STATS_LAST_BLOCK - 1) / SDC_STATS_LAST_BLOCK, 2048);
  hipLaunchKernelGGL(sdc_stats_last_kernel, dim3(blocks), dim3(SDC_STATS_LAST_BLOCK), 0, st, P);
  return hipGetLastError();
}
