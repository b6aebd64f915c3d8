// sdc_actor_grad.hpp -- the gradient of an actor's loss with respect to its parameters, and the PPO loss's derivative per stored
// log-probability: what sdc_actor_backward and sdc_ppo_dlogp (sdc_capi.hip) hand to the four kernels of sdc_actor_grad.hip.  The
// contract: include/sustaindc_hip.h THE ACTORS' GRADIENT.
//
// sdc_actor_grad_tanh_kernel / sdc_actor_grad_relu_kernel (one body, the activation its template parameter; a kernel each, so that a
// launch carries one body's registers).  THE MAPPING IS sdc_actor_eval_kernel's (sdc_actor_eval.hpp): a wavefront takes sixteen rows,
// lane l = (g = l >> 4, e = l & 15) works on row e, and the forward is that kernel's own (sdc_actor_forward.hpp), recomputed per tile
// with a tape: 128 activations per row are cheaper to compute again than to store and fetch.  The backward, per tile:
//   the logits' gradient per row in every lane of its column;
//   dY1 = W2^T dZ2 and dX = W1^T dZ1 with dZ AS IT STANDS in the accumulators as the B operand (sdc_actor_grad_pack.hpp) -- no data moves;
//   dX only when the feature LayerNorm is on (nothing is propagated to the observations);
//   dW2 += dZ2 Y1^T, dW1 += dZ1 X^T and dW3 += Y2 dl^T sum over ROWS: both operands need the rows on the k side, a transpose of what the
//   lanes hold, through the wavefront's own LDS tiles [unit][16 rows] (row stride SDC_AGR_S = 20 dwords: a lane's four rows are one
//   16-byte read, the stores of a lane group fall into distinct banks; Y1^T is stored by the forward itself).  k-step q, k slot g stands
//   for row 4 g + q; lane (g, e) supplies A = dZ[unit 16 t + e][rows 4 g ..] and B = Y[unit 16 t' + e][rows 4 g ..], and register r of
//   accumulator (t, t') is dW[unit 16 t + 4 g + r][input 16 t' + e]: 64 + 32 + 16 accumulation registers that stay in the register file
//   over every pass of the grid-stride loop.  Entry 26 of X's padding is a ONE: that column of dW1 is db1.
//   The other per-unit vectors (b2, the hidden LayerNorms' gains, LayerNorm 1's bias, b3, the feature LayerNorm's pair: 81 registers) are
//   PER-LANE SUMS in the accumulators' layout, added up across the sixteen columns once, at the end; dbeta2 = W3^T db3 is formed there.
// gfx950's 512 registers per lane are 256 that vector instructions address and 256 accumulation registers: the tape, the per-lane sums
// and the working set fill the first, the matrix products' sums sit in the second -- ONE wavefront per SIMD, one workgroup of four per
// CU.  No lane predicate lives across the loop (the compiler keeps each as an SGPR pair): padded LDS rows instead, relu' as arithmetic.
// Per wavefront and pass: 28 + 64 forward and 64 (dY1) + 64 (dW2) + 16 (dW3) + 32 (dW1) + 32 (dX, feature LayerNorm on) backward MFMAs.
//
// THE ORDER OF EVERY SUM IS FIXED, no atomics: a lane's sums take its rows in pass order; the sixteen columns are added by a butterfly
// (xor 1, 2, 4, 8); the matrix instructions sum a tile's rows in the hardware's fixed order; the four wavefronts of a workgroup are
// added in wavefront order through LDS ((w0 + w1) + w2) + w3 into partial [workgroup][SDC_ACTOR_N_PARAMS] of the handle's buffer;
// sdc_actor_grad_reduce_kernel adds the B partials of a parameter in workgroup order in fp64 and rounds once;
// sdc_actor_grad_sq_kernel folds (double)g * (double)g: lane l of ONE workgroup of 256 takes parameters l, l + 256, ... in that order,
// then for half = 128 .. 1 lane l < half takes lane l + half.  B = min(ceil(n_rows / 64), SDC_ACTOR_GRAD_MAX_BLOCKS): n_rows alone.
//
// EVERY ADDRESS A LANE FORMS IS BELOW ITS ARRAY'S END.  With row = row0 + r a dword is loaded only when row < n_rows:
//   obs      row * row_stride + k       <= (n_rows - 1) * row_stride + 25
//   actions  row * action_stride        <= (n_rows - 1) * action_stride         (its VALUE enters a comparison only, never an address)
//   dlogp    row                        <= n_rows - 1
//   part     b * SDC_ACTOR_N_PARAMS + j  < B * SDC_ACTOR_N_PARAMS, j < SDC_ACTOR_N_PARAMS; b = blockIdx < B <= SDC_ACTOR_GRAD_MAX_BLOCKS
//   grads    j < SDC_ACTOR_N_PARAMS
// in 64-bit arithmetic.  LDS: a tile's stores are (16 t + 4 g + i) * 20 + e < 1280, its 16-byte reads (16 t + e) * 20 + 4 g + 3 < 1280; the
// logit-gradient tile: stores g * 20 + e < 80, reads min(e, 3) * 20 + 4 g + 3 < 80 (row 3: zeros); the observation tile: stores
// lane + 64 j < 448, reads e * 26 + 4 s + g <= 417 < 448 (entries 26, 27 read a neighbour's and are dropped); the stage:
// SDC_ACTOR_N_PARAMS dwords inside the tiles.  The number of passes is the same in every wavefront of a workgroup: every barrier is
// reached by all.  A row at or past n_rows computes on zeros with a zero logit gradient: it adds exact zeros.
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

#define SDC_ACTOR_GRAD_BLOCK SDC_ROWMLP_BLOCK                                 // four wavefronts: 64 rows per workgroup and pass
#define SDC_ACTOR_GRAD_BLOCK_ROWS SDC_ROWMLP_BLOCK_ROWS
#define SDC_AGR_S SDC_ROWMLP_TS                                               // 20 dwords between two units' rows in a transposed tile
#define SDC_ACTOR_GRAD_SQ_BLOCK 256                                           // lanes of sdc_actor_grad_sq_kernel (a power of two)

// where each member of sdc_actor_params starts in `grads`
#define SDC_AGR_LN0G 0
#define SDC_AGR_LN0B 26
#define SDC_AGR_W1 52
#define SDC_AGR_B1 (SDC_AGR_W1 + 64 * 26)
#define SDC_AGR_LN1G (SDC_AGR_B1 + 64)
#define SDC_AGR_LN1B (SDC_AGR_LN1G + 64)
#define SDC_AGR_W2 (SDC_AGR_LN1B + 64)
#define SDC_AGR_B2 (SDC_AGR_W2 + 64 * 64)
#define SDC_AGR_LN2G (SDC_AGR_B2 + 64)
#define SDC_AGR_LN2B (SDC_AGR_LN2G + 64)
#define SDC_AGR_W3 (SDC_AGR_LN2B + 64)
#define SDC_AGR_B3 (SDC_AGR_W3 + 3 * 64)
static_assert(SDC_AGR_B3 + 3 == SDC_ACTOR_N_PARAMS, "the members of sdc_actor_params in declaration order");
static_assert(SDC_AGR_W1 * sizeof(float) == offsetof(sdc_actor_params, w1) && SDC_AGR_W2 * sizeof(float) == offsetof(sdc_actor_params, w2) &&
              SDC_AGR_W3 * sizeof(float) == offsetof(sdc_actor_params, w3) && SDC_AGR_B3 * sizeof(float) == offsetof(sdc_actor_params, b3) &&
              SDC_AGR_LN2B * sizeof(float) == offsetof(sdc_actor_params, ln2_beta) && SDC_AGR_LN1G * sizeof(float) == offsetof(sdc_actor_params, ln1_gamma),
              "grads is sdc_actor_params' float members as they lie");

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
struct SdcActorGradReduce {
  int n_part;                  // B
  const float* part;
  float* grads;                // [SDC_ACTOR_N_PARAMS]
};
struct SdcActorGradSq {
  const float* grads;
  double* grad_sq;             // [1]
};
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

static inline int sdc_actor_grad_blocks(const long long n_rows) {
  const long long want = (n_rows + SDC_ACTOR_GRAD_BLOCK_ROWS - 1) / SDC_ACTOR_GRAD_BLOCK_ROWS;
  return (int)(want < SDC_ACTOR_GRAD_MAX_BLOCKS ? want : SDC_ACTOR_GRAD_MAX_BLOCKS);
}

hipError_t sdc_actor_grad_launch(const SdcActorGrad& P, int activation, hipStream_t st);      // activation: sdc_actor_params' (0 tanh, 1 relu)
hipError_t sdc_actor_grad_reduce_launch(const SdcActorGradReduce& P, hipStream_t st);
hipError_t sdc_actor_grad_sq_launch(const SdcActorGradSq& P, hipStream_t st);
hipError_t sdc_ppo_dlogp_launch(const SdcPpoDlogp& P, hipStream_t st);
