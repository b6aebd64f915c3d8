// sdc_actor_eval.hip -- sdc_actor_eval_kernel, sdc_ppo_terms_kernel and sdc_ppo_stats_kernel: one agent's actor over rows of stored
// observations, and the PPO terms (importance ratio, clipped surrogate, the HAPPO factor, their fixed-order fp64 statistics) of the
// log-probabilities that come of it, for sdc_actor_evaluate and sdc_ppo_terms (sdc_capi.hip; the plans, the lane mappings and the
// address bounds: sdc_actor_eval.hpp; the arithmetic: include/sustaindc_hip.h EVALUATE THE ACTORS ON STORED ROWS).
//
// The network is sdc_rowmlp.hpp's, as the critic's (26 inputs in 7 k-steps, three outputs: sdc_actor_forward.hpp), and so is the
// kernel's plumbing.  The PPO terms are fp64 with nothing fused (the library is built with -ffp-contract=off; the pragma below says it
// for this file whatever the flags; the network's last layer names its fmaf itself).
#include <hip/hip_runtime.h>

#include "sdc_actor_eval.hpp"
#include "sdc_actor_forward.hpp"
#include "sdc_rowmlp.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int TILE_DW = sdc_rowmlp::TILE_DW<SDC_AEV_IN>;              // 416
constexpr int TILE_LOADS = sdc_rowmlp::TILE_LOADS<SDC_AEV_IN>;        // 7
static_assert((SDC_PPO_BLOCK & (SDC_PPO_BLOCK - 1)) == 0 && SDC_PPO_BLOCK % 64 == 0, "the tree halves whole wavefronts");

using Lds = sdc_rowmlp::Lds<SdcActorEvalDev, SDC_AEV_IN>;
static_assert(sizeof(Lds) <= 40 * 1024, "four workgroups' LDS fit a CU");

// The forward itself: sdc_actor_forward.hpp (shared with sdc_actor_grad.hip), here with nothing kept.
__device__ __forceinline__ void forward(const SdcActorEvalDev* W, float (&x)[SDC_AEV_S1], const int lane, float (&lg)[SDC_AEV_OUT]) {
  sdc_rowmlp::NoTape none;
  if (__builtin_amdgcn_readfirstlane((W->flags >> 1) & 3) == 1) sdc_aev::forward_kind<1>(W, x, lane, lg, none);
  else sdc_aev::forward_kind<0>(W, x, lane, lg, none);
}

// One pass of a wavefront: the fetched dwords through the wavefront's tile -> the logits of row (lane & 15), in every lane of that
// column; behind the tile's reads the NEXT pass's rows are fetched (the barrier and the order: sdc_critic.hip's pass).
__device__ __forceinline__ void pass(Lds& L, float (&v)[TILE_LOADS], const SdcActorEval& P, const long long next0, const int wave,
                                     const int lane, float (&lg)[SDC_AEV_OUT]) {
#pragma unroll
  for (int j = 0; j < TILE_LOADS; j++) {
    const int u = lane + 64 * j;
    if (u < TILE_DW) L.tile[wave][u] = v[j];
  }
  __syncthreads();
  const int g = lane >> 4, e = lane & 15;
  float x[SDC_AEV_S1];
#pragma unroll
  for (int s = 0; s < SDC_AEV_S1; s++) {
    const int k = 4 * s + g;
    x[s] = 0.0f;
    if (k < SDC_AEV_IN) x[s] = L.tile[wave][e * SDC_AEV_IN + k];
  }
  sdc_rowmlp::fetch<SDC_AEV_IN>(v, P.obs, P.row_stride, next0, P.n_rows, lane);
  forward(&L.net, x, lane, lg);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_ACTOR_EVAL_BLOCK, SDC_ACTOR_EVAL_WAVES_PER_SIMD) sdc_actor_eval_kernel(SdcActorEval P) {
  __shared__ Lds L;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  sdc_rowmlp::to_lds(&L.net, P.actor);
  const long long n_pass = (P.n_rows + SDC_ACTOR_EVAL_BLOCK_ROWS - 1) / SDC_ACTOR_EVAL_BLOCK_ROWS;
  const long long stride = (long long)gridDim.x * SDC_ACTOR_EVAL_BLOCK_ROWS;
  long long row0 = (long long)blockIdx.x * SDC_ACTOR_EVAL_BLOCK_ROWS + wave * SDC_ROWMLP_ROWS;
  float v[TILE_LOADS];
  sdc_rowmlp::fetch<SDC_AEV_IN>(v, P.obs, P.row_stride, row0, P.n_rows, lane);
#pragma unroll 1
  for (long long p = blockIdx.x; p < n_pass; p += gridDim.x, row0 += stride) {
    // (a next pass that does not exist starts at or past n_rows -- the grid's stride is whole workgroups --: fetch loads nothing)
    float lg[SDC_AEV_OUT];
    pass(L, v, P, row0 + stride, wave, lane, lg);
    const long long row = row0 + lane;
    if (lane < SDC_ROWMLP_ROWS && row < P.n_rows) {
      float* const out = P.logits + row * P.logits_stride;
      out[0] = lg[0];
      out[1] = lg[1];
      out[2] = lg[2];
    }
  }
}

// ---- the PPO terms -----------------------------------------------------------------------------------------------------------------
namespace {

// the eight statistics of include/sustaindc_hip.h: four sums, a count, a minimum, a maximum (entry 7, the element count, is the host's)
struct Fold {
  double s[7];
};
__device__ __forceinline__ Fold fold_start() {
  return Fold{{0.0, 0.0, 0.0, 0.0, 0.0, __builtin_huge_val(), -__builtin_huge_val()}};
}
// a takes b: the sums a + b, the minimum b < a ? b : a, the maximum b > a ? b : a
__device__ __forceinline__ void fold_take(Fold& a, const Fold& b) {
#pragma unroll
  for (int q = 0; q < 5; q++) a.s[q] = a.s[q] + b.s[q];
  a.s[5] = b.s[5] < a.s[5] ? b.s[5] : a.s[5];
  a.s[6] = b.s[6] > a.s[6] ? b.s[6] : a.s[6];
}

// the workgroup's SDC_PPO_BLOCK folds halved through LDS into lane 0's (every lane runs every round: the barriers are the workgroup's)
__device__ __forceinline__ void halve(double (&part)[7][SDC_PPO_BLOCK], Fold& f, const int l) {
#pragma unroll
  for (int q = 0; q < 7; q++) part[q][l] = f.s[q];
  __syncthreads();
  for (int half = SDC_PPO_BLOCK / 2; half >= 1; half >>= 1) {
    if (l < half) {
      Fold a, b;
#pragma unroll
      for (int q = 0; q < 7; q++) {
        a.s[q] = part[q][l];
        b.s[q] = part[q][l + half];
      }
      fold_take(a, b);
#pragma unroll
      for (int q = 0; q < 7; q++) part[q][l] = a.s[q];
    }
    __syncthreads();
  }
  if (l == 0) {
#pragma unroll
    for (int q = 0; q < 7; q++) f.s[q] = part[q][0];
  }
}

template <bool STATS>
__device__ __forceinline__ void ppo_pass(const SdcPpoTerms& P, double (&part)[7][SDC_PPO_BLOCK]) {
  const long long stride = (long long)gridDim.x * SDC_PPO_BLOCK;
  const size_t col = (size_t)P.agent;
  Fold f = fold_start();
  for (long long i = (long long)blockIdx.x * SDC_PPO_BLOCK + threadIdx.x; i < P.n; i += stride) {
    const size_t j = (size_t)i * 3 + col;      // (the column is part of the address)
    const double lr = (double)P.new_lp[j] - (double)P.old_lp[j];
    const double r = exp(lr);
    const float rf = (float)r;
    const double A = (double)P.adv[i];
    float ff = 1.0f;
    if (P.factor) ff = P.factor[i];
    const double F = (double)ff;
    const double s1 = r * A;
    double rc = r < P.lo ? P.lo : r;
    rc = rc > P.hi ? P.hi : rc;
    const double s2 = rc * A;
    const double m = s2 < s1 ? s2 : s1;
    const float sf = (float)(F * m);
    P.ratio[i] = rf;
    if (P.surr) P.surr[i] = sf;
    if (P.factor_out) P.factor_out[i] = ff * rf;
    if (STATS) {
      const double rd = (double)rf;
      f.s[0] = f.s[0] + (double)sf;
      f.s[1] = f.s[1] + rd;
      f.s[2] = f.s[2] + lr;
      if (P.entropy) f.s[3] = f.s[3] + (double)P.entropy[j];
      f.s[4] = f.s[4] + ((r < P.lo || r > P.hi) ? 1.0 : 0.0);
      f.s[5] = rd < f.s[5] ? rd : f.s[5];
      f.s[6] = rd > f.s[6] ? rd : f.s[6];
    }
  }
  if (STATS) {
    const int l = (int)threadIdx.x;
    halve(part, f, l);
    if (l == 0) {
      double* const out = P.part + (size_t)blockIdx.x * SDC_PPO_STATS;
#pragma unroll
      for (int q = 0; q < 7; q++) out[q] = f.s[q];
      out[7] = 0.0;
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_PPO_BLOCK) sdc_ppo_terms_kernel(SdcPpoTerms P) {
  __shared__ double part[7][SDC_PPO_BLOCK];
  // (the switch is the launch's, the same in every lane: the barriers of the statistics are reached by all or by none)
  if (P.part) ppo_pass<true>(P, part);
  else ppo_pass<false>(P, part);
}

extern "C" __global__ void __launch_bounds__(SDC_PPO_BLOCK) sdc_ppo_stats_kernel(SdcPpoStats P) {
  __shared__ double part[7][SDC_PPO_BLOCK];
  const int l = (int)threadIdx.x;
  Fold f = fold_start();
  for (int b = l; b < P.n_part; b += SDC_PPO_BLOCK) {
    const double* const src = P.part + (size_t)b * SDC_PPO_STATS;
    Fold x;
#pragma unroll
    for (int q = 0; q < 7; q++) x.s[q] = src[q];
    fold_take(f, x);
  }
  halve(part, f, l);
  if (l == 0) {
#pragma unroll
    for (int q = 0; q < 7; q++) P.stats[q] = f.s[q];
    P.stats[7] = P.count;
  }
}

hipError_t sdc_actor_eval_launch(const SdcActorEval& P, hipStream_t st) {
  const long long passes = (P.n_rows + SDC_ACTOR_EVAL_BLOCK_ROWS - 1) / SDC_ACTOR_EVAL_BLOCK_ROWS;
  const unsigned blocks = (unsigned)(passes < SDC_ACTOR_EVAL_MAX_BLOCKS ? passes : SDC_ACTOR_EVAL_MAX_BLOCKS);
  hipLaunchKernelGGL(sdc_actor_eval_kernel, dim3(blocks), dim3(SDC_ACTOR_EVAL_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_ppo_terms_launch(const SdcPpoTerms& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_ppo_terms_kernel, dim3(sdc_ppo_blocks(P.n)), dim3(SDC_PPO_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_ppo_stats_launch(const SdcPpoStats& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_ppo_stats_kernel, dim3(1), dim3(SDC_PPO_BLOCK), 0, st, P);
  return hipGetLastError();
}
