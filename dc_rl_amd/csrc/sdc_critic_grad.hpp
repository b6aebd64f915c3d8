// sdc_critic_grad.hpp -- the critic's half of an on-policy update: the network's raw output over stored rows, the value loss and its
// derivative per row, and the gradient with respect to the critic's parameters: what sdc_critic_evaluate, sdc_value_loss and
// sdc_critic_backward (sdc_capi.hip) hand to the kernels of sdc_critic_grad.hip.  The contract: include/sustaindc_hip.h THE CRITIC'S
// GRADIENT.
//
// sdc_critic_raw_kernel: sdc_critic_values_kernel's shape and plumbing (sdc_critic.hip: the untaped trunk of sdc_rowmlp.hpp, 64 rows
// per workgroup and pass, the rows fetched densely through the wavefront's tile) and its head without `* scale + shift`:
// u = all_sum(unit_dot(w3, h)) + b3, the value sdc_critic::forward rounds before it scales it.
//
// sdc_value_loss_kernel: elementwise, ONE LANE PER ELEMENT in grid-stride, sdc_ppo_terms_kernel's plan word for word: B = min(ceil(n /
// 256), SDC_PPO_MAX_BLOCKS) workgroups of 256 lanes, lane l of workgroup b takes elements i = b * 256 + l + k * 256 * B; with `stats`
// the lane folds its elements into seven fp64 values in that order, the workgroup halves them through LDS (half = 128 .. 1) into
// partial b of the handle's [SDC_PPO_MAX_BLOCKS][8], and sdc_ppo_stats_kernel (sdc_actor_eval.hip, as it stands) folds the partials.
//
// sdc_critic_grad_tanh_kernel / sdc_critic_grad_relu_kernel (one body, the activation its template parameter; a kernel each).  THE
// PLAN, THE MAPPING, THE ORDER OF EVERY SUM AND THE LDS BOUNDS ARE THE SHARED BACKWARD'S (sdc_rowmlp_grad.hpp) with 29 inputs, the
// forward sdc_rowmlp::trunk<KIND, 29> with a Tape<8> (32 + 64 MFMAs).  The critic's own, in its head (sdc_critic_grad.hip):
//   the head has ONE output, so with c_r = dvalue[r]: dy2 = w3 c, db3 = sum c, and the three sums over rows that remain are products
//   of ONE per-lane sum S[u] = sum_r c_r n2[u][r] (n2: the second hidden LayerNorm's normalised values):
//       dgain2 = w3 S        dbeta2 = w3 db3        dW3 = sum_r c_r (n2 gain2 + beta2) = gain2 S + beta2 db3
//   formed once per wavefront at the end.  dW3 as a PRODUCT, not a per-lane sum of c y2 (sixteen more registers and 32 more
//   instructions per pass) nor the actors' matrix product (a third transposed tile): S is summed anyway, the products round twice more
//   per wavefront where a per-lane sum rounds once per row, and doubling c doubles S and with it all three exactly.
// B = min(ceil(n_rows / 64), SDC_CRITIC_GRAD_MAX_BLOCKS).
//
// EVERY ADDRESS A LANE FORMS IS BELOW ITS ARRAY'S END.  With row = row0 + r, r < 16, a dword is loaded or stored only when row < n_rows:
//   share_obs   row0 * 29 + u, u = lane + 64 j < (rows that exist) * 29       <= (n_rows - 1) * 29 + 28
//   dvalue      row                                                            <= n_rows - 1
//   raw_values  row                                                            <= n_rows - 1
//   value loss  i < n for raw_values, value_preds, returns, loss, dvalue; part b * 8 + q, b = blockIdx < B <= SDC_PPO_MAX_BLOCKS, q < 8
// in 64-bit arithmetic.  LDS: the raw kernel's tile: stores u < 464 under its test, reads e * 29 + k, k < 29.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"
#include "sdc_actor_eval.hpp"
#include "sdc_critic.hpp"
#include "sdc_critic_grad_pack.hpp"
#include "sdc_rowmlp_grad.hpp"

#define SDC_CRITIC_GRAD_BLOCK SDC_ROWMLP_BLOCK                                // four wavefronts: 64 rows per workgroup and pass
#define SDC_CRITIC_GRAD_SQ_BLOCK 256                                          // lanes of sdc_critic_grad_sq_kernel (a power of two)
#define SDC_VALUE_LOSS_HUBER 1                                                // sdc_value_loss' flags
#define SDC_VALUE_LOSS_CLIPPED 2

// where each member of sdc_critic_params starts in `grads`
using SdcCriticGradAt = SdcRowMlpGradAt<SDC_CRITIC_IN, 1>;
static_assert(SdcCriticGradAt::N == SDC_CRITIC_N_PARAMS, "the members of sdc_critic_params in declaration order");
static_assert(SdcCriticGradAt::W1 * sizeof(float) == offsetof(sdc_critic_params, w1) && SdcCriticGradAt::W2 * sizeof(float) == offsetof(sdc_critic_params, w2) &&
              SdcCriticGradAt::W3 * sizeof(float) == offsetof(sdc_critic_params, w3) && SdcCriticGradAt::B3 * sizeof(float) == offsetof(sdc_critic_params, b3) &&
              SdcCriticGradAt::LN2B * sizeof(float) == offsetof(sdc_critic_params, ln2_b) &&
              SdcCriticGradAt::LN1G * sizeof(float) == offsetof(sdc_critic_params, ln1_g) &&
              SdcCriticGradAt::B1 * sizeof(float) == offsetof(sdc_critic_params, b1),
              "grads is sdc_critic_params' float members as they lie");
static_assert(SDC_CRITIC_GRAD_SQ_BLOCK == SDC_ROWMLP_GRAD_SQ_BLOCK, "one sum-of-squares plan");

struct SdcCriticRaw {
  const SdcCriticDev* critic;
  const float* rows;           // [n_rows][29], dword-aligned
  long long n_rows;
  float* raw;                  // [n_rows]
};
struct SdcValueLoss {
  long long n;
  const float* raw;            // [n] the network's raw output u
  const float* vp;             // [n] the stored (normalised) value predictions
  const float* ret;            // [n] the returns
  double scale, shift;         // the target's ValueNorm: t = (ret - shift) / scale
  double clip, delta, coef;
  int flags;                   // SDC_VALUE_LOSS_*
  float* loss;                 // [n] or nullptr
  float* dvalue;               // [n]
  double* part;                // [B][8], or nullptr: no statistics
};
struct SdcCriticGrad {
  const SdcCriticDev* critic;
  const SdcCriticGradDev* critic_t;
  const float* rows;           // [n_rows][29]
  long long n_rows;
  const float* dvalue;         // [n_rows]
  float* part;                 // [B][SDC_CRITIC_N_PARAMS]
};
using SdcCriticGradReduce = SdcRowMlpGradReduce;
using SdcCriticGradSq = SdcRowMlpGradSq;

hipError_t sdc_critic_raw_launch(const SdcCriticRaw& P, hipStream_t st);
hipError_t sdc_value_loss_launch(const SdcValueLoss& P, hipStream_t st);
hipError_t sdc_critic_grad_launch(const SdcCriticGrad& P, int activation, hipStream_t st);      // activation: 0 tanh, 1 relu
hipError_t sdc_critic_grad_reduce_launch(const SdcCriticGradReduce& P, hipStream_t st);
hipError_t sdc_critic_grad_sq_launch(const SdcCriticGradSq& P, hipStream_t st);
