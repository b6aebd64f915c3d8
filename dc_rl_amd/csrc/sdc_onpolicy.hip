// sdc_onpolicy.hip -- sdc_gae_kernel, sdc_adv_moments_kernel and sdc_action_logp_kernel: a collected rollout's rewards, dones, values,
// actions and logits -> the returns, advantages, masks, normalised value predictions, advantage moments and action log-probabilities of
// an on-policy training batch, for sdc_gae and sdc_action_log_probs (sdc_capi.hip; the plans, the lane mappings and the address
// bounds: sdc_onpolicy.hpp).
//
// The arithmetic is the one include/sustaindc_hip.h states for the two calls, operation by operation: the recurrence in fp32 in the
// reference's order, the moments and the log-probabilities in fp64, nothing fused (the library is built with -ffp-contract=off; the
// pragma below says it for this file whatever the flags).  The log-probability's arithmetic is sdc_policy_stats.hip's `fold`, RESTATED
// here and not shared: moving that kernel's body into a common function would put its register allocation and schedule (88 VGPRs at
// four wavefronts per SIMD, sdc_policy_stats.hip) at the inliner's mercy for no gain in this one.
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_onpolicy.hpp"
#include "sdc_stats.hpp"

#pragma clang fp contract(off)

namespace {

static_assert(SDC_GAE_BLOCK == SDC_WAVE, "one wavefront per workgroup");
static_assert((SDC_MOMENTS_BLOCK & (SDC_MOMENTS_BLOCK - 1)) == 0 && SDC_MOMENTS_BLOCK % SDC_WAVE == 0, "the tree halves whole wavefronts");
static_assert(SDC_N_AGENTS == 3, "an env's three rewards, an element's three logits");

typedef double f64x2 __attribute__((ext_vector_type(2)));

// what a lane loads for one step
struct Step {
  float r, v;
  unsigned char d;
};

// the lane's state over the walk
struct Walk {
  float run;        // use_gae: gae; otherwise the running return
  float vnext;      // V[t+1]
  double s1, s2;    // the sum and the sum of squares of its advantages so far
};

// STEPS steps downwards from step t, all the loads in flight together; o: the lane's entry of step t in a [T][N] array
template <int STEPS>
__device__ __forceinline__ void take(Step (&s)[STEPS], const SdcGae& P, const size_t o, const size_t N) {
#pragma unroll
  for (int i = 0; i < STEPS; i++) {
    const size_t k = o - (size_t)i * N;
    s[i].r = P.rew[k * 3 + (size_t)P.reward_agent];
    s[i].d = P.done[k];
    s[i].v = P.values[k];
  }
}

// one step of the recurrence and its stores; o: the lane's dword offset of step t in a [T][N] array (a [T+1][N] array's row t + 1 is N
// further)
template <bool GAE, bool PREDS>
__device__ __forceinline__ void fold(Walk& W, const Step& s, const SdcGae& P, const size_t o, const size_t N, const float scale,
                                     const float shift) {
  const float r = s.r;
  const float m = s.d ? 0.0f : 1.0f;
  float ret;
  if (GAE) {
    const float delta = (r + (P.g * W.vnext) * m) - s.v;
    W.run = delta + (P.c * m) * W.run;
    ret = W.run + s.v;
  } else {
    W.run = (W.run * P.g) * m + r;
    ret = W.run;
  }
  const float adv = ret - s.v;
  P.returns[o] = ret;
  P.advantages[o] = adv;
  P.masks[o + N] = m;
  if (PREDS) P.value_preds[o] = (s.v - shift) / scale;
  const double a = (double)adv;
  W.s1 += a;
  W.s2 += a * a;
  W.vnext = s.v;
}

template <bool GAE, bool PREDS>
__device__ __forceinline__ void walk(const SdcGae& P, const size_t n) {
  const size_t N = (size_t)P.n_envs, T = (size_t)P.steps;
  float scale = 1.0f, shift = 0.0f;
  if (PREDS) {
    scale = P.critic->scale;
    shift = P.critic->shift;
  }
  // the bootstrap row
  const float vT = P.values[T * N + n];
  if (PREDS) P.value_preds[T * N + n] = (vT - shift) / scale;
  Walk W = {GAE ? 0.0f : vT, vT, 0.0, 0.0};
  size_t o = (T - 1) * N + n;      // the lane's entry of step T - 1 in a [T][N] array; a step down is N entries less

  size_t left = T;
#pragma unroll 1
  for (; left >= SDC_STATS_UNROLL; left -= SDC_STATS_UNROLL) {
    Step s[SDC_STATS_UNROLL];
    take(s, P, o, N);
#pragma unroll
    for (int i = 0; i < SDC_STATS_UNROLL; i++) fold<GAE, PREDS>(W, s[i], P, o - (size_t)i * N, N, scale, shift);
    o -= (size_t)SDC_STATS_UNROLL * N;      // (behind step 0 the offset has wrapped and is not used)
  }
#pragma unroll 1
  for (; left > 0; left--) {
    Step s[1];
    take(s, P, o, N);
    fold<GAE, PREDS>(W, s[0], P, o, N, scale, shift);
    o -= N;
  }

  const bool first = P.first_done != nullptr && P.first_done[n] != 0;
  P.masks[n] = first ? 0.0f : 1.0f;
  *reinterpret_cast<f64x2*>(P.adv_part + n * 2) = f64x2{W.s1, W.s2};
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_GAE_BLOCK) sdc_gae_kernel(SdcGae P) {
  const size_t n = (size_t)blockIdx.x * SDC_GAE_BLOCK + threadIdx.x;
  if (n >= (size_t)P.n_envs) return;      // (no barrier below: the missing lanes of the last wavefront leave)
  // (both switches are the launch's, the same in every lane: four bodies, one taken)
  if (P.use_gae) {
    if (P.value_preds) walk<true, true>(P, n);
    else walk<true, false>(P, n);
  } else {
    if (P.value_preds) walk<false, true>(P, n);
    else walk<false, false>(P, n);
  }
}

extern "C" __global__ void __launch_bounds__(SDC_MOMENTS_BLOCK) sdc_adv_moments_kernel(SdcAdvMoments P) {
  __shared__ f64x2 part[SDC_MOMENTS_BLOCK];
  const int l = threadIdx.x;
  f64x2 s = {0.0, 0.0};
  for (int n = l; n < P.n_envs; n += SDC_MOMENTS_BLOCK) {
    const f64x2 x = *reinterpret_cast<const f64x2*>(P.adv_part + (size_t)n * 2);
    s.x += x.x;
    s.y += x.y;
  }
  part[l] = s;
  __syncthreads();
  for (int half = SDC_MOMENTS_BLOCK / 2; half >= 1; half >>= 1) {      // (every lane runs every round: the barriers are the workgroup's)
    if (l < half) {
      const f64x2 a = part[l], b = part[l + half];
      part[l] = f64x2{a.x + b.x, a.y + b.y};
    }
    __syncthreads();
  }
  if (l == 0) {
    const f64x2 t = part[0];
    const double mean = t.x / P.count;
    const double var = t.y / P.count - mean * mean;
    *reinterpret_cast<f64x2*>(P.moments) = f64x2{mean, sqrt(var > 0.0 ? var : 0.0)};
  }
}

namespace {

template <bool ENTROPY>
__device__ __forceinline__ void logp_pass(const SdcActionLogp& P) {
  const long long stride = (long long)gridDim.x * SDC_LOGP_BLOCK;
  for (long long i = (long long)blockIdx.x * SDC_LOGP_BLOCK + threadIdx.x; i < P.n; i += stride) {
    const float* const l = P.logits + (size_t)i * 3;
    const float l0 = l[0], l1 = l[1], l2 = l[2];
    const int j = P.actions[i];
    float m = l0;
    m = l1 > m ? l1 : m;
    m = l2 > m ? l2 : m;
    const double z0 = (double)l0 - (double)m, z1 = (double)l1 - (double)m, z2 = (double)l2 - (double)m;
    const double e0 = exp(z0), e1 = exp(z1), e2 = exp(z2);
    const double sum = (e0 + e1) + e2;
    const double lse = log(sum);
    const double lp0 = z0 - lse, lp1 = z1 - lse, lp2 = z2 - lse;
    P.log_probs[i] = (float)(j == 0 ? lp0 : (j == 1 ? lp1 : lp2));
    if (ENTROPY) {
      const double p0 = e0 / sum, p1 = e1 / sum, p2 = e2 / sum;
      P.entropy[i] = (float)(-((p0 * lp0 + p1 * lp1) + p2 * lp2));
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_LOGP_BLOCK) sdc_action_logp_kernel(SdcActionLogp P) {
  if (P.entropy) logp_pass<true>(P);
  else logp_pass<false>(P);
}

hipError_t sdc_gae_launch(const SdcGae& P, hipStream_t st) {
  const int blocks = (P.n_envs + SDC_GAE_BLOCK - 1) / SDC_GAE_BLOCK;
  hipLaunchKernelGGL(sdc_gae_kernel, dim3(blocks), dim3(SDC_GAE_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_adv_moments_launch(const SdcAdvMoments& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_adv_moments_kernel, dim3(1), dim3(SDC_MOMENTS_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_action_logp_launch(const SdcActionLogp& P, hipStream_t st) {
  const long long want = (P.n + SDC_LOGP_BLOCK - 1) / SDC_LOGP_BLOCK;
  const int blocks = (int)(want < SDC_LOGP_MAX_BLOCKS ? want : SDC_LOGP_MAX_BLOCKS);
  hipLaunchKernelGGL(sdc_action_logp_kernel, dim3(blocks), dim3(SDC_LOGP_BLOCK), 0, st, P);
  return hipGetLastError();
}
