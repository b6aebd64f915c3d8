// sdc_policy_stats.hip -- sdc_policy_stats_kernel: a rollout chunk's actions and logits -> per-(env, agent) policy statistics (how often
// each action was played, how often the action changed from one step to the next, the last action, the summed log-probability of
// the actions played and the summed entropy of the distributions) for sdc_rollout_actor_stats (sdc_capi.hip; the plan, the lane mapping
// and the address bounds: sdc_policy_stats.hpp).
//
// The arithmetic is the one include/sustaindc_hip.h states for sdc_rollout_actor_stats, operation by operation: the maximum in fp32 by
// comparisons and selects, everything behind it in fp64 without fused multiply-adds (the library is built with -ffp-contract=off; the
// pragma below says it for this file whatever the flags), the steps in order.  A chunk that is not the call's first continues from
// what the chunk before it stored.
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_policy_stats.hpp"
#include "sdc_stats.hpp"

#pragma clang fp contract(off)

namespace {

static_assert(SDC_POLICY_BLOCK % SDC_WAVE == 0, "whole wavefronts per workgroup");
static_assert(SDC_POLICY_COUNTS == 5 && SDC_POLICY_N0 == 0 && SDC_POLICY_N1 == 1 && SDC_POLICY_N2 == 2 && SDC_POLICY_SWITCHES == 3 &&
                  SDC_POLICY_LAST == 4,
              "the counts");
static_assert(SDC_POLICY_SUMS == 2 && SDC_POLICY_LOGP == 0 && SDC_POLICY_ENTROPY == 1, "the sums");

typedef double f64x2 __attribute__((ext_vector_type(2)));

// a lane's statistics
struct Acc {
  int n0, n1, n2, switches, last;
  double logp, entropy;
};

// a lane's twelve bytes of logits and its action of one step
struct Step {
  float l0, l1, l2;
  int j;
};

__device__ __forceinline__ void fold(Acc& A, const Step& s) {
  const int j = s.j;
  A.n0 += j == 0 ? 1 : 0;
  A.n1 += j == 1 ? 1 : 0;
  A.n2 += j == 2 ? 1 : 0;
  A.switches += (A.last >= 0 && j != A.last) ? 1 : 0;
  A.last = j;
  float m = s.l0;
  m = s.l1 > m ? s.l1 : m;
  m = s.l2 > m ? s.l2 : m;
  const double z0 = (double)s.l0 - (double)m, z1 = (double)s.l1 - (double)m, z2 = (double)s.l2 - (double)m;
  const double e0 = exp(z0), e1 = exp(z1), e2 = exp(z2);
  const double sum = (e0 + e1) + e2;
  const double lse = log(sum);
  const double lp0 = z0 - lse, lp1 = z1 - lse, lp2 = z2 - lse;
  const double p0 = e0 / sum, p1 = e1 / sum, p2 = e2 / sum;
  A.logp += j == 0 ? lp0 : (j == 1 ? lp1 : lp2);
  A.entropy += -((p0 * lp0 + p1 * lp1) + p2 * lp2);
}

// STEPS consecutive steps of this lane, all the loads in flight together
template <int STEPS>
__device__ __forceinline__ void take(Step (&v)[STEPS], const float* const lp, const int32_t* const ap, const size_t lstep, const size_t astep) {
#pragma unroll
  for (int i = 0; i < STEPS; i++) {
    const float* const l = lp + (size_t)i * lstep;
    v[i].l0 = l[0];
    v[i].l1 = l[1];
    v[i].l2 = l[2];
    v[i].j = ap[(size_t)i * astep];
  }
}

}  // namespace

// (amdgpu_waves_per_eu: left alone, the scheduler -- ordering for instruction-level parallelism, dc_rl_amd/_lib.py -- interleaves the
// unrolled steps' sixteen exp / log sequences and takes 222 VGPRs, two wavefronts per SIMD; held to four it takes 88, without spills)
extern "C" __global__ void __launch_bounds__(SDC_POLICY_BLOCK) __attribute__((amdgpu_waves_per_eu(SDC_POLICY_WAVES_PER_EU)))
sdc_policy_stats_kernel(SdcPolicyStats P) {
  const size_t lanes = (size_t)P.n_envs * SDC_N_AGENTS;
  const size_t t = (size_t)blockIdx.x * SDC_POLICY_BLOCK + threadIdx.x;
  if (t >= lanes) return;      // (no barrier below: the missing lanes of the last wavefront leave)
  // this lane's addresses at step 0, and what a step adds
  const int32_t* ap = P.actions + t;
  const float* lp = P.logits + t * 3;
  const size_t astep = lanes, lstep = lanes * 3;
  int32_t* const cnt = P.counts + t * SDC_POLICY_COUNTS;
  f64x2* const sums = reinterpret_cast<f64x2*>(P.sums + t * SDC_POLICY_SUMS);

  Acc A = {0, 0, 0, 0, -1, 0.0, 0.0};
  if (!P.init) {
    A.n0 = cnt[SDC_POLICY_N0];
    A.n1 = cnt[SDC_POLICY_N1];
    A.n2 = cnt[SDC_POLICY_N2];
    A.switches = cnt[SDC_POLICY_SWITCHES];
    A.last = cnt[SDC_POLICY_LAST];
    const f64x2 s = *sums;
    A.logp = s.x;
    A.entropy = s.y;
  }

  int k = 0;
#pragma unroll 1
  for (; k + SDC_STATS_UNROLL <= P.steps; k += SDC_STATS_UNROLL) {
    Step v[SDC_STATS_UNROLL];
    take(v, lp, ap, lstep, astep);
#pragma unroll
    for (int i = 0; i < SDC_STATS_UNROLL; i++) fold(A, v[i]);
    lp += (size_t)SDC_STATS_UNROLL * lstep;
    ap += (size_t)SDC_STATS_UNROLL * astep;
  }
#pragma unroll 1
  for (; k < P.steps; k++) {
    Step v[1];
    take(v, lp, ap, lstep, astep);
    fold(A, v[0]);
    lp += lstep;
    ap += astep;
  }

  cnt[SDC_POLICY_N0] = A.n0;
  cnt[SDC_POLICY_N1] = A.n1;
  cnt[SDC_POLICY_N2] = A.n2;
  cnt[SDC_POLICY_SWITCHES] = A.switches;
  cnt[SDC_POLICY_LAST] = A.last;
  *sums = f64x2{A.logp, A.entropy};
}

hipError_t sdc_policy_stats_launch(const SdcPolicyStats& P, hipStream_t st) {
  const size_t lanes = (size_t)P.n_envs * SDC_N_AGENTS;
  const int blocks = (int)((lanes + SDC_POLICY_BLOCK - 1) / SDC_POLICY_BLOCK);
  hipLaunchKernelGGL(sdc_policy_stats_kernel, dim3(blocks), dim3(SDC_POLICY_BLOCK), 0, st, P);
  return hipGetLastError();
}
