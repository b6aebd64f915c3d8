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
// Mapping.  The rows are independent and there are thousands to millions of them, so -- unlike the actors (sdc_actor.hpp), which sit
// between two env-steps of the two or four envs their wavefront owns -- a wavefront takes SIXTEEN rows and a hidden layer is the
// TRANSPOSED product H^T = W X^T on v_mfma_f32_16x16x4_f32 (exact fp32: per output a k-ordered fmaf chain):
//     D[unit i][row j] += A[i][k] B[k][j]     lane l = (g = l >> 4, e = l & 15) supplies A[i = e][k = g] and B[k = g][j = e],
//                                             and holds D[i = 4 g + r][j = e] in accumulator register r
// The 64 units go on the A side in four tiles t of 16: four independent accumulators (the instruction issues every 32 cycles and a
// dependent one waits 40).  Accumulator register (t, i) of lane (g, e) is unit 16 t + 4 g + i of row e, and THAT REGISTER IS the B
// operand of layer 2's k-step s = 4 t + i: the host numbers W2's columns so (sdc_critic_pack.hpp), and the layer-to-layer hand-over
// moves no data.  A operands are weights: one 16-byte LDS read per lane and k-step serves the four tiles (24 reads per 16 rows).  The
// per-unit vectors (bias, LayerNorm gain and bias, w3) come as four 16-byte reads each, laid out per lane group.
// A row's LayerNorm(64) and its last layer are sums over the lane's 16 registers and then across the four lane groups g -- the four
// DPP rows of the wavefront: v_permlane16_swap / v_permlane32_swap (sdc_actor.hpp's swap16_sum / swap32_sum) all-reduce them; each
// column e keeps its own row.  The order of every sum is fixed by (t, i, g) alone: a row's value does not depend on its column, its
// wavefront or the rows next to it.
// Numerics are sdc_actor.hpp's: tanh through exp2 / rcp (sdc_act::activate), the hidden LayerNorms' moments of values shifted by one
// unit's value (its comment says why a ReLU needs that), rsq(var + eps) with var clamped at 0 -- a dead layer gives beta, no NaN.
// Cost per wavefront and 16 rows: 32 + 64 MFMAs of 32 cycles, 24 + 32 LDS reads of 16 bytes, ~640 other vector instructions
// (measurements and what bounds the kernel: DESIGN.md section 4.24).
#pragma once
#include "sdc_actor.hpp"
#include "sdc_critic_pack.hpp"

namespace sdc_critic {

using sdc_act::f4;
using sdc_act::spread16;
using sdc_act::swap16_sum;
using sdc_act::swap32_sum;

// ACROSS the four lane groups, every column e on its own.  Two values at once: rows [a0+a1, b0+b1, a2+a3, b2+b3], then
// [A, B, A, B], then each spread over all four rows -- three swaps and two adds for the two moments of a LayerNorm.
__device__ __forceinline__ void all_sum2(const float a, const float b, float& A, float& B) {
  const float t = swap16_sum(a, b);
  spread16(swap32_sum(t, t), A, B);
}
__device__ __forceinline__ float all_sum(const float a) {
  const float t = swap16_sum(a, a);
  return swap32_sum(t, t);
}
// lane group 0's value in every lane group (rows [v0, v0, v2, v2], then the lower half twice)
__device__ __forceinline__ float group0(const float v) {
  float even, odd;
  spread16(v, even, odd);
  const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(even), __float_as_uint(even), false, false);
  return __uint_as_float(s[0]);
}

// the lane's 16 entries of a per-unit vector: v[g][t][0..3]
__device__ __forceinline__ void unit_vector(f4 (&v)[4], const float (&src)[4][4][4], const int g) {
#pragma unroll
  for (int t = 0; t < 4; t++) v[t] = *reinterpret_cast<const f4*>(src[g][t]);
}

// activation and LayerNorm(64) of a layer's pre-activations (the bias went in as the accumulators' start): acc[t][i] in, h in place.
// One pass over SHIFTED values d = v - v[unit 0] (sdc_actor.hpp epilogue).
template <int KIND>
__device__ __forceinline__ void epilogue(f4 (&acc)[4], const float (&gain)[4][4][4], const float (&bias)[4][4][4], const int g) {
  float s1 = 0.0f, s2 = 0.0f;
  const float v0 = group0(sdc_act::activate<KIND>(acc[0][0]));
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float d = sdc_act::activate<KIND>(acc[t][i]) - v0;
      acc[t][i] = d;
      s1 += d;
      s2 += d * d;
    }
  float sum, sq;
  all_sum2(s1, s2, sum, sq);
  const float mean = sum * (1.0f / SDC_CRITIC_H);
  const float var = fmaxf(sq * (1.0f / SDC_CRITIC_H) - mean * mean, 0.0f);
  const float rs = __builtin_amdgcn_rsqf(var + 1e-5f);
  f4 gn[4], bs[4];
  unit_vector(gn, gain, g);
  unit_vector(bs, bias, g);
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) acc[t][i] = (acc[t][i] - mean) * rs * gn[t][i] + bs[t][i];
}

// W: the critic in LDS.  x[s]: lane (g, e) holds entry 4 s + g of row e's share_obs (0 beyond entry 28, and for a row past the
// batch's last).  -> the row's value, in every lane of column e.
template <int KIND>
__device__ __forceinline__ float forward_kind(const SdcCriticDev* W, float (&x)[SDC_CRITIC_S1], const int lane) {
  const int g = lane >> 4;
  // feature LayerNorm (share_obs entries are of order one -- normalised by construction --: one unshifted pass, as the actors')
  if (W->flags & 1) {
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int s = 0; s < SDC_CRITIC_S1; s++) {
      s1 += x[s];
      s2 += x[s] * x[s];
    }
    float sum, sq;
    all_sum2(s1, s2, sum, sq);
    const float mean = sum * (1.0f / SDC_CRITIC_IN);
    const float var = fmaxf(sq * (1.0f / SDC_CRITIC_IN) - mean * mean, 0.0f);
    const float rs = __builtin_amdgcn_rsqf(var + 1e-5f);
#pragma unroll
    for (int s = 0; s < SDC_CRITIC_S1; s++) x[s] = (x[s] - mean) * rs * W->ln0_g[g][s] + W->ln0_b[g][s];      // (gain and bias 0 beyond entry 28)
  }
  // ---- layer 1: 29 (32) -> 64 ------------------------------------------------------------------------------------------------------
  f4 h[4];
  unit_vector(h, W->b1, g);
#pragma unroll
  for (int s = 0; s < SDC_CRITIC_S1; s++) {
    const f4 a = *reinterpret_cast<const f4*>(W->a1[s][lane]);
#pragma unroll
    for (int t = 0; t < 4; t++) h[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], x[s], h[t], 0, 0, 0);
  }
  epilogue<KIND>(h, W->ln1_g, W->ln1_b, g);
  // ---- layer 2: 64 -> 64; k-step s = 4 t + i reads register (t, i) of layer 1 ------------------------------------------------------
  f4 acc[4];
  unit_vector(acc, W->b2, g);
#pragma unroll
  for (int s = 0; s < SDC_CRITIC_S2; s++) {
    const f4 a = *reinterpret_cast<const f4*>(W->a2[s][lane]);
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], h[s >> 2][s & 3], acc[t], 0, 0, 0);
  }
  epilogue<KIND>(acc, W->ln2_g, W->ln2_b, g);
  // ---- the value: 64 -> 1 ----------------------------------------------------------------------------------------------------------
  f4 w3[4];
  unit_vector(w3, W->w3, g);
  float v = 0.0f;
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) v = fmaf(w3[t][i], acc[t][i], v);
  return (all_sum(v) + W->b3) * W->scale + W->shift;
}
// (the activation is a template parameter, as the actors': chosen per element it is a branch around every exp -> rcp chain)
__device__ __forceinline__ float forward(const SdcCriticDev* W, float (&x)[SDC_CRITIC_S1], const int lane) {
  if (__builtin_amdgcn_readfirstlane((W->flags >> 1) & 3) == 1) return forward_kind<1>(W, x, lane);
  return forward_kind<0>(W, x, lane);
}

}  // namespace sdc_critic

// ---- the kernels' plans (sdc_critic.hip) ------------------------------------------------------------------------------------------
#define SDC_CRITIC_BLOCK 256                                            // four wavefronts: 64 rows per workgroup and pass
#define SDC_CRITIC_BLOCK_ROWS (SDC_CRITIC_BLOCK / 64 * SDC_CRITIC_ROWS)
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
