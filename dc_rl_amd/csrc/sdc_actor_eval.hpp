// sdc_actor_eval.hpp -- the actors over STORED rows, and the PPO terms built from their log-probabilities: what sdc_actor_evaluate and
// sdc_ppo_terms (sdc_capi.hip) hand to the three kernels of sdc_actor_eval.hip.  The contract: include/sustaindc_hip.h EVALUATE THE
// ACTORS ON STORED ROWS.
//
// sdc_actor_eval_kernel: one agent's network (sdc_actor.hpp's header comment: LayerNorm(26) under flag bit 0 -> Linear(26, 64) -> act ->
// LayerNorm(64) -> Linear(64, 64) -> act -> LayerNorm(64) -> Linear(64, 3), tanh or relu) over R rows that lie `row_stride` floats apart,
// the three logits of a row `logits_stride` floats apart.  THE MAPPING IS sdc_rowmlp.hpp's, the critic's, not the rollout's: sixteen rows
// per wavefront on the matrix cores, every sum's order fixed by the unit's place alone -- a row's logits do not depend on its lane
// column, its wavefront, the rows next to it, the strides or n_rows.  The forward: sdc_actor_forward.hpp.
// Workgroups of four wavefronts copy the agent's SdcActorEvalDev (26 KB) to LDS once, then take 64 rows per pass and as many passes as
// the grid (at most SDC_ACTOR_EVAL_MAX_BLOCKS workgroups) leaves them (sdc_rowmlp.hpp's plumbing).  A wavefront's 16 rows are 416
// dwords, NOT contiguous under a stride: lane l takes tile dwords u = l, l + 64, ... (7 loads, u < 416), dword u being entry k = u % 26
// of tile row r = u / 26 at address obs + (row0 + r) * row_stride + k.
//
// EVERY ADDRESS A LANE FORMS IS BELOW ITS ARRAY'S END.  With row = row0 + r a dword is loaded only when row < n_rows (a row at or past
// n_rows is not loaded: its tile entries are 0, it computes on zeros and stores nothing), and then
//   obs      row * row_stride + k          <=  (n_rows - 1) * row_stride + 25      (k <= 25; the caller's array holds that many floats + 1)
//   logits   row * logits_stride + c       <=  (n_rows - 1) * logits_stride + 2    (c <= 2; stored by lane e < 16 of the wavefront)
// in 64-bit arithmetic.  The tile's reads stay inside the tile: e * 26 + k < 416 with k = 4 s + g < 26 (beyond: 0, nothing read).  The
// number of passes is the same in every wavefront of a workgroup (it follows from blockIdx alone): the barrier of a pass is reached by all.
//
// sdc_ppo_terms_kernel / sdc_ppo_stats_kernel: elementwise, ONE LANE PER (STEP, ENV) in grid-stride, B = min(ceil(n / 256),
// SDC_PPO_MAX_BLOCKS) workgroups of 256 lanes -- a function of n = T N alone.  Lane l of workgroup b takes elements
// i = b * 256 + l + k * 256 * B, k = 0, 1, ...: dword 3 i + agent (< 3 n) of new_log_probs, old_log_probs and entropy -- the column is
// part of the address, never a choice among three loaded dwords --, dword i (< n) of advantages and factor, and stores dword i of ratio,
// surr and factor_out (the element's own: factor_out may be factor).  With `stats` the lane folds its elements into eight fp64 values in
// that order, the workgroup halves them through LDS (entry l takes entry l + half, half = 128 .. 1) into part[b][8] (< 8 B doubles of
// the handle's [SDC_PPO_MAX_BLOCKS][8]); sdc_ppo_stats_kernel, ONE workgroup of 256 lanes: lane l folds partials l, l + 256, ... < B in
// that order, the same halving, lane 0 stores stats[0..7].  No atomics; without `stats` neither reduction runs.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sustaindc_hip.h"
#include "sdc_actor_eval_pack.hpp"
#include "sdc_rowmlp.hpp"

#define SDC_ACTOR_EVAL_BLOCK SDC_ROWMLP_BLOCK                                 // four wavefronts: 64 rows per workgroup and pass
#define SDC_ACTOR_EVAL_BLOCK_ROWS SDC_ROWMLP_BLOCK_ROWS
#define SDC_ACTOR_EVAL_WAVES_PER_SIMD 4                                       // the register budget: four workgroups per CU, as their LDS allows
#define SDC_ACTOR_EVAL_MAX_BLOCKS 1024                                        // ... of 256 CUs, all resident at once; more rows: more passes
#define SDC_PPO_BLOCK 256                                                     // lanes per workgroup of both kernels (a power of two)
#define SDC_PPO_MAX_BLOCKS 1024                                               // stage 1's cap: B = min(ceil(T N / 256), this)
#define SDC_PPO_STATS 8

struct SdcActorEval {
  const SdcActorEvalDev* actor;
  const float* obs;            // row r: 26 floats at obs + r * row_stride
  long long row_stride;        // >= 26
  long long n_rows;
  float* logits;               // row r: 3 floats at logits + r * logits_stride
  long long logits_stride;     // >= 3
};

struct SdcPpoTerms {
  long long n;                 // T N
  int agent;                   // the column of the [T][N][3] arrays, 0 .. 2
  const float* new_lp;         // [T][N][3]
  const float* old_lp;         // [T][N][3]
  const float* entropy;        // [T][N][3] or nullptr
  const float* adv;            // [T][N]
  const float* factor;         // [T][N] or nullptr (1)
  double lo, hi;               // 1 - clip_param, 1 + clip_param
  float* ratio;                // [T][N]
  float* surr;                 // [T][N] or nullptr
  float* factor_out;           // [T][N] or nullptr; may be `factor`
  double* part;                // [B][8], or nullptr: no statistics
};

struct SdcPpoStats {
  int n_part;                  // B
  double count;                // T N
  const double* part;          // [B][8]
  double* stats;               // [8]
};

static inline int sdc_ppo_blocks(const long long n) {
  const long long want = (n + SDC_PPO_BLOCK - 1) / SDC_PPO_BLOCK;
  return (int)(want < SDC_PPO_MAX_BLOCKS ? want : SDC_PPO_MAX_BLOCKS);
}

hipError_t sdc_actor_eval_launch(const SdcActorEval& P, hipStream_t st);
hipError_t sdc_ppo_terms_launch(const SdcPpoTerms& P, hipStream_t st);
hipError_t sdc_ppo_stats_launch(const SdcPpoStats& P, hipStream_t st);
