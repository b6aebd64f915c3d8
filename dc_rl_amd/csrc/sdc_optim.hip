// sdc_optim.hip -- sdc_adam_update_kernel, sdc_adam_gather_kernel and sdc_critic_norm_kernel: one Adam step with gradient-norm clipping
// over a network's master parameters and the rewrite of every packed copy the other kernels read, for sdc_actor_adam_step /
// sdc_critic_adam_step, and the critic's scale and shift for sdc_set_critic_norm (sdc_capi.hip; the plan, the lane mapping and the address bounds: sdc_optim_dev.hpp;
// the arithmetic, shared with a host compiler: sdc_optim.hpp; the contract: include/sustaindc_hip.h THE OPTIMISER STEP).
//
// fp32 per element with nothing fused (the library is built with -ffp-contract=off; the pragma below says it for this file whatever
// the flags), division and square root correctly rounded (hipcc's default for fp32); the sum of squares and the scalars are fp64.
#include <hip/hip_runtime.h>

#include "sdc_optim_dev.hpp"

#pragma clang fp contract(off)

namespace {

// phases: 1 the update (sum of squares, scalars, elements), 2 the gather (after a skipped step it rewrites every dword with the bits it
// holds), 3 both behind each other on one workgroup (the measured alternative: sdc_optim_dev.hpp)
template <int PHASES>
__device__ __forceinline__ void adam_step(const SdcAdamStep& P) {
  __shared__ double part[SDC_ADAM_SQ_LANES];
  __shared__ SdcAdamScalars k;
  __shared__ int go;
  const int l = (int)threadIdx.x;
  if (PHASES & 1) {
    if (l < SDC_ADAM_SQ_LANES) part[l] = sdc_adam_lane_sq(P.grads, P.n, l);
    __syncthreads();
    for (int half = SDC_ADAM_SQ_LANES / 2; half >= 1; half >>= 1) {
      if (l < half) part[l] = part[l] + part[l + half];
      __syncthreads();
    }
    if (l == 0) {
      const double S = part[0];
      if (P.grad_norm) P.grad_norm[0] = sqrt(S);
      sdc_optim_state st = *P.state;
      SdcAdamScalars ks;
      const bool stepped = sdc_adam_prepare(P.adam, S, st, ks);
      *P.state = st;
      if (stepped) k = ks;
      go = stepped ? 1 : 0;
    }
    __syncthreads();
    if (go) {
      const SdcAdamScalars ks = k;
      for (int j = P.first + l; j < P.n; j += SDC_ADAM_BLOCK) {
        float p = P.params[j], m = P.m[j], v = P.v[j];
        sdc_adam_element(ks, P.grads[j], p, m, v);
        P.params[j] = p;
        P.m[j] = m;
        P.v[j] = v;
      }
    }
  }
  if (PHASES == 3) {
    __syncthreads();      // (the workgroup's stores to params above are visible to its loads below)
    if (!go) return;
  }
  if (PHASES & 2) {
    const uint32_t* const src = reinterpret_cast<const uint32_t*>(P.params);
    const int stride = (int)(gridDim.x * SDC_ADAM_BLOCK);
    int at = 0;
    for (int i = 0; i < P.n_packs; i++) {
      const int32_t* const table = P.table + at;
      uint32_t* const dst = P.pack[i];
      const int n = P.pack_dwords[i];
      for (int d = (int)blockIdx.x * SDC_ADAM_BLOCK + l; d < n; d += stride) {
        const int32_t t = table[d];
        if (t >= 0) dst[d] = src[t];
      }
      at += n;
    }
  }
}

}  // namespace

#ifdef SDC_OPTIM_ONE_LAUNCH
extern "C" __global__ void __launch_bounds__(SDC_ADAM_BLOCK) sdc_adam_step_kernel(SdcAdamStep P) { adam_step<3>(P); }
#else
extern "C" __global__ void __launch_bounds__(SDC_ADAM_BLOCK) sdc_adam_update_kernel(SdcAdamStep P) { adam_step<1>(P); }
extern "C" __global__ void __launch_bounds__(SDC_ADAM_BLOCK) sdc_adam_gather_kernel(SdcAdamStep P) { adam_step<2>(P); }
#endif

extern "C" __global__ void __launch_bounds__(64) sdc_critic_norm_kernel(SdcCriticNorm P) {
  if (threadIdx.x == 0) {
    P.critic->scale = P.scale;
    P.critic->shift = P.shift;
  }
}

hipError_t sdc_adam_step_launch(const SdcAdamStep& P, hipStream_t st) {
#ifdef SDC_OPTIM_ONE_LAUNCH
  hipLaunchKernelGGL(sdc_adam_step_kernel, dim3(1), dim3(SDC_ADAM_BLOCK), 0, st, P);
#else
  hipLaunchKernelGGL(sdc_adam_update_kernel, dim3(1), dim3(SDC_ADAM_BLOCK), 0, st, P);
  hipLaunchKernelGGL(sdc_adam_gather_kernel, dim3(SDC_ADAM_GATHER_BLOCKS), dim3(SDC_ADAM_BLOCK), 0, st, P);
#endif
  return hipGetLastError();
}

hipError_t sdc_critic_norm_launch(const SdcCriticNorm& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_critic_norm_kernel, dim3(1), dim3(64), 0, st, P);
  return hipGetLastError();
}
