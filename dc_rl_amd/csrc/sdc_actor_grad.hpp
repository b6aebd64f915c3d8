// sdc_actor_grad.hpp -- the gradient of an actor's loss with respect to its parameters, and the PPO loss's derivative per stored
// log-probability: what sdc_actor_backward and sdc_ppo_dlogp (sdc_capi.hip) hand to the kernels of sdc_actor_grad.hip.  The
// contract: include/sustaindc_hip.h THE ACTORS' GRADIENT.
//
// sdc_actor_grad_tanh_kernel / sdc_actor_grad_relu_kernel (one body, the activation its template parameter; a kernel each, so that a
// launch carries one body's registers).  THE PLAN, THE MAPPING, THE ORDER OF EVERY SUM AND THE LDS BOUNDS ARE THE SHARED BACKWARD'S
// (sdc_rowmlp_grad.hpp) with 26 inputs, the forward sdc_actor_forward.hpp's.  The actors' own, in their head (sdc_actor_grad.hip):
//   the logits' gradient per row in every lane of its column;
//   dW3 += Y2 dl^T as a third matrix product over rows, through two more of the wavefront's LDS tiles (Y2^T, and the logits' gradient
//   [c][row] with a fourth row of zeros): 16 more accumulation registers, 16 more MFMAs per wavefront and pass (28 + 64 forward);
//   LayerNorm 2's gain and b3 as per-lane sums; dbeta2 = W3^T db3 is formed at the end.
// B = min(ceil(n_rows / 64), SDC_ACTOR_GRAD_MAX_BLOCKS).
//
// EVERY ADDRESS A LANE FORMS IS BELOW ITS ARRAY'S END.  With row = row0 + r a dword is loaded only when row < n_rows:
//   obs      row * row_stride + k       <= (n_rows - 1) * row_stride + 25
//   actions  row * action_stride        <= (n_rows - 1) * action_stride         (its VALUE enters a comparison only, never an address)
//   dlogp    row                        <= n_rows - 1
// in 64-bit arithmetic.  LDS: the logit-gradient tile: stores g * 20 + e < 80, reads min(e, 3) * 20 + 4 g + 3 < 80 (row 3: zeros); Y2^T
// is a transposed tile as the shared ones.
//
// sdc_ppo_dlogp_kernel: elementwise, one lane per (step, env) in grid-stride as sdc_ppo_terms_kernel, the agent's column part of the
// load address.  (It lives in sdc_actor_grad.hip: sdc_actor_eval.hip is gated on holding exactly its three kernels.)
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"
#include "sdc_actor_eval.hpp"
#include "sdc_actor_forward.hpp"
#include "sdc_actor_grad_pack.hpp"
#include "sdc_rowmlp_grad.hpp"

#define SDC_ACTOR_GRAD_BLOCK SDC_ROWMLP_BLOCK                                 // four wavefronts: 64 rows per workgroup and pass
#define SDC_ACTOR_GRAD_SQ_BLOCK 256                                           // lanes of sdc_actor_grad_sq_kernel (a power of two)

// where each member of sdc_actor_params starts in `grads`
using SdcActorGradAt = SdcRowMlpGradAt<SDC_AEV_IN, SDC_AEV_OUT>;
static_assert(SdcActorGradAt::N == SDC_ACTOR_N_PARAMS, "the members of sdc_actor_params in declaration order");
static_assert(SdcActorGradAt::W1 * sizeof(float) == offsetof(sdc_actor_params, w1) && SdcActorGradAt::W2 * sizeof(float) == offsetof(sdc_actor_params, w2) &&
              SdcActorGradAt::W3 * sizeof(float) == offsetof(sdc_actor_params, w3) && SdcActorGradAt::B3 * sizeof(float) == offsetof(sdc_actor_params, b3) &&
              SdcActorGradAt::LN2B * sizeof(float) == offsetof(sdc_actor_params, ln2_beta) &&
              SdcActorGradAt::LN1G * sizeof(float) == offsetof(sdc_actor_params, ln1_gamma),
              "grads is sdc_actor_params' float members as they lie");
static_assert(SDC_ACTOR_GRAD_SQ_BLOCK == SDC_ROWMLP_GRAD_SQ_BLOCK, "one sum-of-squares plan");

struct SdcActorGrad {
  const SdcActorEvalDev* actor;
  const SdcActorGradDev* actor_t;
  const float* obs;            // row r: 26 floats at obs + r * row_stride
  long long row_stride;        // >= 26
  long long n_rows;
  const int32_t* actions;      // row r: actions[r * action_stride]
  long long action_stride;     // >= 1
  const float* dlogp;          // [n_rows]
  double dent;
  float* part;                 // [B][SDC_ACTOR_N_PARAMS]
};
using SdcActorGradReduce = SdcRowMlpGradReduce;
using SdcActorGradSq = SdcRowMlpGradSq;
struct SdcPpoDlogp {
  long long n;                 // T N
  int agent;
  const float* new_lp;         // [T][N][3]
  const float* old_lp;         // [T][N][3]
  const float* adv;            // [T][N]
  const float* factor;         // [T][N] or nullptr (1)
  double lo, hi, scale;
  float* dlogp;                // [T][N]
};

hipError_t sdc_actor_grad_launch(const SdcActorGrad& P, int activation, hipStream_t st);      // activation: sdc_actor_params' (0 tanh, 1 relu)
hipError_t sdc_actor_grad_reduce_launch(const SdcActorGradReduce& P, hipStream_t st);
hipError_t sdc_actor_grad_sq_launch(const SdcActorGradSq& P, hipStream_t st);
hipError_t sdc_ppo_dlogp_launch(const SdcPpoDlogp& P, hipStream_t st);
