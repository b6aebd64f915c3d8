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
// MAPPING AND THE BACKWARD ARE sdc_actor_grad.hpp's, written next to it for 29 inputs and a head of one output: a wavefront takes
// sixteen rows, lane l = (g = l >> 4, e = l & 15) works on row e, the forward is sdc_rowmlp::trunk<KIND, 29> recomputed per tile with a
// Tape<8>; per tile
//   dY1 = W2^T dZ2 and dX = W1^T dZ1 with dZ AS IT STANDS in the accumulators as the B operand (sdc_critic_grad_pack.hpp); dX only when
//   the feature LayerNorm is on (nothing is propagated to share_obs);
//   dW2 += dZ2 Y1^T and dW1 += dZ1 X^T through the wavefront's transposed LDS tiles [unit][16 rows] (row stride SDC_ROWMLP_TS = 20
//   dwords; Y1^T is stored by the forward itself) into 64 + 32 accumulation registers kept over the grid-stride loop; entry 29 of X's
//   padding (entries 29 .. 31 are free) is a ONE: that column of dW1 is db1;
//   the head has ONE output, so with c_r = dvalue[r]: dy2 = w3 c, db3 = sum c, and the three sums over rows that remain are products
//   of ONE per-lane sum S[u] = sum_r c_r n2[u][r] (n2: the second hidden LayerNorm's normalised values):
//       dgain2 = w3 S        dbeta2 = w3 db3        dW3 = sum_r c_r (n2 gain2 + beta2) = gain2 S + beta2 db3
//   formed once per wavefront at the end.  dW3 as a PRODUCT, not a per-lane sum of c y2 (sixteen more registers and 32 more
//   instructions per pass) nor the actors' matrix product (a third transposed tile): S is summed anyway, the products round twice more
//   per wavefront where a per-lane sum rounds once per row, and doubling c doubles S and with it all three exactly.
//   The other per-unit vectors (b2, LayerNorm 1's pair, b3, the feature LayerNorm's pair) are per-lane sums in the accumulators'
//   layout, added across the sixteen columns once, at the end.
// ONE wavefront per SIMD, one workgroup of four per CU, as the actors' kernel.  No lane predicate lives across the loop: the
// observation tile is padded to 512 dwords and every lane stores all its eight, relu' is arithmetic (sdc_rowmlp.hpp).
// Per wavefront and pass: 32 + 64 forward and 64 (dY1) + 64 (dW2) + 32 (dW1) + 32 (dX, feature LayerNorm on) backward MFMAs.
//
// THE ORDER OF EVERY SUM IS FIXED, no atomics: a lane's sums take its rows in pass order; the sixteen columns are added by a butterfly
// (xor 1, 2, 4, 8); the matrix instructions sum a tile's rows in the hardware's fixed order; the four wavefronts of a workgroup are
// added in wavefront order through LDS ((w0 + w1) + w2) + w3 into partial [workgroup][SDC_CRITIC_N_PARAMS] of the handle's buffer;
// sdc_critic_grad_reduce_kernel adds the B partials of a parameter in workgroup order in fp64 and rounds once;
// sdc_critic_grad_sq_kernel folds (double)g * (double)g as sdc_actor_grad_sq_kernel does: lane l of ONE workgroup of 256 takes
// parameters l, l + 256, ... in that order, then for half = 128 .. 1 lane l < half takes lane l + half.
// B = min(ceil(n_rows / 64), SDC_CRITIC_GRAD_MAX_BLOCKS): n_rows alone.
//
// EVERY ADDRESS A LANE FORMS IS BELOW ITS ARRAY'S END.  With row = row0 + r, r < 16, a dword is loaded or stored only when row < n_rows:
//   share_obs   row0 * 29 + u, u = lane + 64 j < (rows that exist) * 29       <= (n_rows - 1) * 29 + 28
//   dvalue      row                                                            <= n_rows - 1
//   raw_values  row                                                            <= n_rows - 1
//   value loss  i < n for raw_values, value_preds, returns, loss, dvalue; part b * 8 + q, b = blockIdx < B <= SDC_PPO_MAX_BLOCKS, q < 8
//   part        b * SDC_CRITIC_N_PARAMS + j < B * SDC_CRITIC_N_PARAMS, j < SDC_CRITIC_N_PARAMS; b = blockIdx < B <= SDC_CRITIC_GRAD_MAX_BLOCKS
//   grads       j < SDC_CRITIC_N_PARAMS
// in 64-bit arithmetic.  LDS: a transposed tile's stores are (16 t + 4 g + i) * 20 + e < 1280 (X^T: (4 s + g) * 20 + e, 4 s + g <= 31:
// < 640), its 16-byte reads (16 t + e) * 20 + 4 g + 3 < 1280; the gradient kernel's observation tile: stores lane + 64 j < 512, reads
// e * 29 + 4 s + g <= 15 * 29 + 31 = 466 < 512 (entries 29 .. 31 read a neighbour's or fetch's zeros and are dropped); the raw kernel's
// tile: stores u < 464 under its test, reads e * 29 + k, k < 29; the stage: SDC_CRITIC_N_PARAMS dwords inside the tiles.  The number of
// passes is the same in every wavefront of a workgroup: every barrier is reached by all.  A row at or past n_rows computes on zeros
// with a zero coefficient: it adds exact zeros.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"
#include "sdc_actor_eval.hpp"
#include "sdc_critic.hpp"
#include "sdc_critic_grad_pack.hpp"

#define SDC_CRITIC_GRAD_BLOCK SDC_ROWMLP_BLOCK                                // four wavefronts: 64 rows per workgroup and pass
#define SDC_CRITIC_GRAD_BLOCK_ROWS SDC_ROWMLP_BLOCK_ROWS
#define SDC_CRITIC_GRAD_SQ_BLOCK 256                                          // lanes of sdc_critic_grad_sq_kernel (a power of two)
#define SDC_VALUE_LOSS_HUBER 1                                                // sdc_value_loss' flags
#define SDC_VALUE_LOSS_CLIPPED 2

// where each member of sdc_critic_params starts in `grads`
#define SDC_CGR_LN0G 0
#define SDC_CGR_LN0B 29
#define SDC_CGR_W1 58
#define SDC_CGR_B1 (SDC_CGR_W1 + 64 * 29)
#define SDC_CGR_LN1G (SDC_CGR_B1 + 64)
#define SDC_CGR_LN1B (SDC_CGR_LN1G + 64)
#define SDC_CGR_W2 (SDC_CGR_LN1B + 64)
#define SDC_CGR_B2 (SDC_CGR_W2 + 64 * 64)
#define SDC_CGR_LN2G (SDC_CGR_B2 + 64)
#define SDC_CGR_LN2B (SDC_CGR_LN2G + 64)
#define SDC_CGR_W3 (SDC_CGR_LN2B + 64)
#define SDC_CGR_B3 (SDC_CGR_W3 + 64)
static_assert(SDC_CGR_B3 + 1 == SDC_CRITIC_N_PARAMS, "the members of sdc_critic_params in declaration order");
static_assert(SDC_CGR_W1 * sizeof(float) == offsetof(sdc_critic_params, w1) && SDC_CGR_W2 * sizeof(float) == offsetof(sdc_critic_params, w2) &&
              SDC_CGR_W3 * sizeof(float) == offsetof(sdc_critic_params, w3) && SDC_CGR_B3 * sizeof(float) == offsetof(sdc_critic_params, b3) &&
              SDC_CGR_LN2B * sizeof(float) == offsetof(sdc_critic_params, ln2_b) && SDC_CGR_LN1G * sizeof(float) == offsetof(sdc_critic_params, ln1_g) &&
              SDC_CGR_B1 * sizeof(float) == offsetof(sdc_critic_params, b1),
              "grads is sdc_critic_params' float members as they lie");

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
struct SdcCriticGradReduce {
  int n_part;                  // B
  const float* part;
  float* grads;                // [SDC_CRITIC_N_PARAMS]
};
struct SdcCriticGradSq {
  const float* grads;
  double* grad_sq;             // [1]
};

static inline int sdc_critic_grad_blocks(const long long n_rows) {
  const long long want = (n_rows + SDC_CRITIC_GRAD_BLOCK_ROWS - 1) / SDC_CRITIC_GRAD_BLOCK_ROWS;
  return (int)(want < SDC_CRITIC_GRAD_MAX_BLOCKS ? want : SDC_CRITIC_GRAD_MAX_BLOCKS);
}

hipError_t sdc_critic_raw_launch(const SdcCriticRaw& P, hipStream_t st);
hipError_t sdc_value_loss_launch(const SdcValueLoss& P, hipStream_t st);
hipError_t sdc_critic_grad_launch(const SdcCriticGrad& P, int activation, hipStream_t st);      // activation: 0 tanh, 1 relu
hipError_t sdc_critic_grad_reduce_launch(const SdcCriticGradReduce& P, hipStream_t st);
hipError_t sdc_critic_grad_sq_launch(const SdcCriticGradSq& P, hipStream_t st);
