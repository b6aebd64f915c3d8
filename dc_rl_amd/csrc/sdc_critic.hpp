// sdc_critic.hpp -- the V critic over rows of share_obs: the reference's VNet (harl/models/value_function_models/v_net.py over
// harl/models/base/mlp.py MLPBase) and ValueNorm.denormalize (harl/common/valuenorm.py), a batched fp32 forward on the matrix cores:
//     x (29, a share_obs row)
//       -> LayerNorm(29)                                   (use_feature_normalization: flags bit 0)
//       -> Linear(29, 64) -> act -> LayerNorm(64)          (hidden_sizes [64, 64]; tanh or relu)
//       -> Linear(64, 64) -> act -> LayerNorm(64)
//       -> Linear(64, 1)  -> v * scale + shift             (the host folds a ValueNorm into scale / shift)
// ONE forward function, sdc_critic::forward, under two kernels (sdc_critic.hip): sdc_critic_values_kernel (rows in, values out) and
// sdc_critic_terminal_kernel (the planners' terminal value) -- the same row gives the same bits under both.
//
// The network, its mapping on the matrix cores, the numerics and the cost: sdc_rowmlp.hpp, with IN = 29 in S1 = 8 k-steps; this file
// adds the head.
#pragma once
#include "sdc_critic_pack.hpp"
#include "sdc_rowmlp.hpp"

namespace sdc_critic {

// W: the critic in LDS.  x[s]: lane (g, e) holds entry 4 s + g of row e's share_obs (0 beyond entry 28, and for a row past the
// batch's last).  -> the row's value, in every lane of column e.
template <int KIND>
__device__ __forceinline__ float forward_kind(const SdcCriticDev* W, float (&x)[SDC_CRITIC_S1], const int lane) {
  sdc_rowmlp::NoTape none;
  sdc_rowmlp::f4 acc[4];
  sdc_rowmlp::trunk<KIND, SDC_CRITIC_IN>(W, x, lane, acc, none);
  const float v = sdc_rowmlp::unit_dot(W->w3, acc, lane >> 4);
  return (sdc_rowmlp::all_sum(v) + W->b3) * W->scale + W->shift;
}
__device__ __forceinline__ float forward(const SdcCriticDev* W, float (&x)[SDC_CRITIC_S1], const int lane) {
  if (__builtin_amdgcn_readfirstlane((W->flags >> 1) & 3) == 1) return forward_kind<1>(W, x, lane);
  return forward_kind<0>(W, x, lane);
}

}  // namespace sdc_critic

// ---- the kernels' plans (sdc_critic.hip) ------------------------------------------------------------------------------------------
#define SDC_CRITIC_BLOCK SDC_ROWMLP_BLOCK                               // four wavefronts: 64 rows per workgroup and pass
#define SDC_CRITIC_BLOCK_ROWS SDC_ROWMLP_BLOCK_ROWS
#define SDC_CRITIC_WAVES_PER_SIMD 4                                     // the register budget: four workgroups per CU, as their LDS allows
#define SDC_CRITIC_MAX_BLOCKS 1024                                      // ... of 256 CUs, all resident at once; more rows: more passes

struct SdcCriticValues {
  const SdcCriticDev* critic;
  const float* rows;       // [n_rows][29], dword-aligned
  long long n_rows;
  float* values;           // [n_rows]
};
struct SdcCriticTerminal {
  const SdcCriticDev* critic;
  const float* rows;       // [n_envs][29]: the share_obs rows of the horizon's last step in the plan block
  const uint8_t* done;     // [n_envs]: that step's
  int n_envs;
  double factor;           // (g[n_steps - 1] * gamma) * weight, multiplied on the host
  double* score;           // [n_envs] this candidate's
};

hipError_t sdc_critic_values_launch(const SdcCriticValues& P, hipStream_t st);
hipError_t sdc_critic_terminal_launch(const SdcCriticTerminal& P, hipStream_t st);
