// sdc_rowmlp.hpp -- the fp32 network over INDEPENDENT ROWS, sixteen rows per wavefront on the matrix cores, that the critic
// (sdc_critic.hpp: 29 inputs, one value) and the stored-row actors (sdc_actor_forward.hpp: 26 inputs, three logits; evaluated by
// sdc_actor_eval.hip, differentiated by sdc_actor_grad.hip) run, and the kernel plumbing around it:
//     x (IN entries of a row)
//       -> LayerNorm(IN)                                   (flags bit 0)
//       -> Linear(IN, 64) -> act -> LayerNorm(64)          (tanh or relu: flags bits 1-2)
//       -> Linear(64, 64) -> act -> LayerNorm(64)          = the TRUNK; the last layer is its caller's, made of unit_dot and all_sum(2)
//
// Mapping.  The rows are independent and there are thousands to millions of them, so -- unlike the closed-loop actors (sdc_actor.hpp),
// which sit between two env-steps of the two or four envs their wavefront owns -- a wavefront takes SIXTEEN rows and a hidden layer is
// the TRANSPOSED product H^T = W X^T on v_mfma_f32_16x16x4_f32 (exact fp32: per output a k-ordered fmaf chain):
//     D[unit i][row j] += A[i][k] B[k][j]     lane l = (g = l >> 4, e = l & 15) supplies A[i = e][k = g] and B[k = g][j = e],
//                                             and holds D[i = 4 g + r][j = e] in accumulator register r
// The 64 units go on the A side in four tiles t of 16: four independent accumulators (the instruction issues every 32 cycles and a
// dependent one waits 40).  Accumulator register (t, i) of lane (g, e) is unit 16 t + 4 g + i of row e, and THAT REGISTER IS the B
// operand of layer 2's k-step s = 4 t + i: the host numbers W2's columns so (sdc_rowmlp_pack.hpp), and the layer-to-layer hand-over
// moves no data.  A operands are weights: one 16-byte LDS read per lane and k-step serves the four tiles.  The per-unit vectors (bias,
// LayerNorm gain and bias, a row of the last layer) come as four 16-byte reads each, laid out per lane group.
// A row's LayerNorm(64) and its last layer are sums over the lane's 16 registers and then across the four lane groups g -- the four
// DPP rows of the wavefront: v_permlane16_swap / v_permlane32_swap (sdc_actor.hpp's swap16_sum / swap32_sum) all-reduce them; each
// column e keeps its own row.  THE ORDER OF EVERY SUM IS FIXED BY THE UNIT'S PLACE (t, i, g) ALONE: what a row gives does not depend
// on its column, its wavefront, the rows next to it, or on which of the kernels runs it.
// Numerics are sdc_actor.hpp's: tanh through exp2 / rcp (sdc_act::activate), the hidden LayerNorms' one-pass moments of values shifted
// by one unit's value (its comment says why a ReLU needs that), rsq(var + eps) with var clamped at 0 -- a dead layer gives beta, no
// NaN; the feature LayerNorm one unshifted pass (the entries are of order one).
// Cost per wavefront and 16 rows: 4 S1 + 64 MFMAs of 32 cycles, S1 + 16 + 24 LDS reads of 16 bytes, ~640 other vector instructions
// (measurements and what bounds the kernels: DESIGN.md sections 4.24, 4.27 and 4.28; this header: 4.29).
//
// With a Tape the same operations in the same order (a row's outputs are the same bits) leave behind, per lane (g, e) and in the
// accumulators' layout, what a backward reads:
//   l0.n[s], l0.rs           the feature LayerNorm's normalised entries (x - mean) * rs and its rs (untouched when the LayerNorm is off)
//   l1, l2: dact, n, rs      the activation's derivative from the forward's own values (tanh' = 1 - h^2, relu' = [z > 0]), the hidden
//                            LayerNorm's normalised values and its rs
//   y2                       the second hidden LayerNorm's output: the last layer's input
//   y1t                      IN: the wavefront's LDS tile that receives the first hidden LayerNorm's output TRANSPOSED, [unit][row],
//                            SDC_ROWMLP_TS dwords between two units (sixteen registers that need not live through layer 2)
// and x[] holds layer 1's input (the feature LayerNorm's output when it is on) on return, with or without a tape.
#pragma once
#include "sdc_actor.hpp"
#include "sdc_rowmlp_pack.hpp"

#define SDC_ROWMLP_BLOCK 256                                            // four wavefronts: 64 rows per workgroup and pass
#define SDC_ROWMLP_BLOCK_ROWS (SDC_ROWMLP_BLOCK / 64 * SDC_ROWMLP_ROWS)
#define SDC_ROWMLP_TS 20      // dwords between two units' sixteen rows in a transposed tile: a lane's four rows are one 16-byte read

namespace sdc_rowmlp {

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
// the lane's share of one output of the last layer: an fmaf chain over its 16 units in the order (t, i)
__device__ __forceinline__ float unit_dot(const float (&w)[4][4][4], const f4 (&h)[4], const int g) {
  f4 w3[4];
  unit_vector(w3, w, g);
  float v = 0.0f;
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) v = fmaf(w3[t][i], h[t][i], v);
  return v;
}

// a lane's sixteen registers (unit 16 t + 4 g + i of row e) into a wavefront's transposed tile: [unit][row]
__device__ __forceinline__ void transpose_out(float* tile, const f4 (&v)[4], const int g, const int e) {
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) tile[(16 * t + 4 * g + i) * SDC_ROWMLP_TS + e] = v[t][i];
}

// ---- the tape ----------------------------------------------------------------------------------------------------------------------
struct Nothing {};
struct NoTape {
  Nothing l0, l1, l2;
};
template <int S1>
struct KeptInput {
  float n[S1], rs;
};
struct KeptHidden {
  f4 dact[4], n[4];
  float rs;
};
template <int S1>
struct Tape {
  KeptInput<S1> l0;
  KeptHidden l1, l2;
  f4 y2[4];
  float* y1t;
};

// the feature LayerNorm over the IN entries of the row that the lane groups hold as x[s] = entry 4 s + g (gain and bias 0 beyond IN - 1)
template <int IN, int S1, class KEPT>
__device__ __forceinline__ void feature_norm(float (&x)[S1], const float (&gain)[4][8], const float (&bias)[4][8], const int g, KEPT& kept) {
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int s = 0; s < S1; s++) {
    s1 += x[s];
    s2 += x[s] * x[s];
  }
  float sum, sq;
  all_sum2(s1, s2, sum, sq);
  const float mean = sum * (1.0f / IN);
  const float var = fmaxf(sq * (1.0f / IN) - mean * mean, 0.0f);
  const float rs = __builtin_amdgcn_rsqf(var + 1e-5f);
  if constexpr (!__is_same(KEPT, Nothing)) kept.rs = rs;
#pragma unroll
  for (int s = 0; s < S1; s++) {
    const float n = (x[s] - mean) * rs;
    if constexpr (!__is_same(KEPT, Nothing)) kept.n[s] = n;
    x[s] = n * gain[g][s] + bias[g][s];
  }
}

// activation and LayerNorm(64) of a layer's pre-activations (the bias went in as the accumulators' start): acc[t][i] in, h in place.
// One pass over SHIFTED values d = v - v[unit 0] (sdc_actor.hpp epilogue).
template <int KIND, class KEPT>
__device__ __forceinline__ void epilogue(f4 (&acc)[4], const float (&gain)[4][4][4], const float (&bias)[4][4][4], const int g, KEPT& kept) {
  constexpr bool KEEP = !__is_same(KEPT, Nothing);
  float s1 = 0.0f, s2 = 0.0f;
  const float v0 = group0(sdc_act::activate<KIND>(acc[0][0]));
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float a = sdc_act::activate<KIND>(acc[t][i]);
      if constexpr (KEEP) {
        // relu' = [z > 0] = [a > 0] as arithmetic (a >= 0; the smallest positive a times 2^252 is above one): no lane mask to keep
        if constexpr (KIND == 1) kept.dact[t][i] = fminf((a * 0x1p+126f) * 0x1p+126f, 1.0f);
        else kept.dact[t][i] = 1.0f - a * a;
      }
      const float d = a - v0;
      acc[t][i] = d;
      s1 += d;
      s2 += d * d;
    }
  float sum, sq;
  all_sum2(s1, s2, sum, sq);
  const float mean = sum * (1.0f / SDC_ROWMLP_H);
  const float var = fmaxf(sq * (1.0f / SDC_ROWMLP_H) - mean * mean, 0.0f);
  const float rs = __builtin_amdgcn_rsqf(var + 1e-5f);
  if constexpr (KEEP) kept.rs = rs;
  f4 gn[4], bs[4];
  unit_vector(gn, gain, g);
  unit_vector(bs, bias, g);
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float n = (acc[t][i] - mean) * rs;
      if constexpr (KEEP) kept.n[t][i] = n;
      acc[t][i] = n * gn[t][i] + bs[t][i];
    }
}

// W: the network in LDS (a device struct of sdc_rowmlp_pack.hpp's trunk).  x[s]: lane (g, e) holds entry 4 s + g of row e (0 beyond
// entry IN - 1, and for a row past the batch's last).  -> acc: the second hidden LayerNorm's output, register (t, i) = unit 16 t + 4 g + i.
// (the activation is a template parameter, as the closed loop's: chosen per element it is a branch around every exp -> rcp chain)
template <int KIND, int IN, int S1, class DEV, class TAPE>
__device__ __forceinline__ void trunk(const DEV* W, float (&x)[S1], const int lane, f4 (&acc)[4], TAPE& tape) {
  constexpr bool TAPED = !__is_same(TAPE, NoTape);
  const int g = lane >> 4;
  if (W->flags & 1) feature_norm<IN>(x, W->ln0_g, W->ln0_b, g, tape.l0);
  // ---- layer 1: IN (4 S1) -> 64 ----------------------------------------------------------------------------------------------------
  f4 h[4];
  unit_vector(h, W->b1, g);
#pragma unroll
  for (int s = 0; s < S1; s++) {
    const f4 a = *reinterpret_cast<const f4*>(W->a1[s][lane]);
#pragma unroll
    for (int t = 0; t < 4; t++) h[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], x[s], h[t], 0, 0, 0);
  }
  epilogue<KIND>(h, W->ln1_g, W->ln1_b, g, tape.l1);
  if constexpr (TAPED) transpose_out(tape.y1t, h, g, lane & 15);
  // ---- layer 2: 64 -> 64; k-step s = 4 t + i reads register (t, i) of layer 1 ------------------------------------------------------
  unit_vector(acc, W->b2, g);
#pragma unroll
  for (int s = 0; s < SDC_ROWMLP_S2; s++) {
    const f4 a = *reinterpret_cast<const f4*>(W->a2[s][lane]);
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], h[s >> 2][s & 3], acc[t], 0, 0, 0);
  }
  epilogue<KIND>(acc, W->ln2_g, W->ln2_b, g, tape.l2);
  if constexpr (TAPED) {
#pragma unroll
    for (int t = 0; t < 4; t++) tape.y2[t] = acc[t];
  }
}

// ---- the kernels' plumbing ---------------------------------------------------------------------------------------------------------
// Workgroups of four wavefronts copy the network from device memory to LDS once, then take 64 rows per pass, 16 per wavefront, and as
// many passes as the grid leaves them.  A wavefront's rows are fetched ahead into registers, go through the wavefront's own LDS tile
// (dword u = entry u % IN of tile row u / IN) and are picked from there as the B operands.  What is shared stands here; the tile's
// store and pick and the pass loop stand in each .hip file, in one function with its fetch and its forward: as helpers of their own
// they are simplified before those are inlined next to them, the compiler then forms their LDS addresses from other expressions and
// schedules the whole kernel anew (DESIGN.md section 4.29 has the trial) -- the kernels are held to the instructions they had.
template <int IN>
constexpr int TILE_DW = SDC_ROWMLP_ROWS * IN;
template <int IN>
constexpr int TILE_LOADS = (TILE_DW<IN> + 63) / 64;      // lane l takes tile dwords l, l + 64, ...

template <class T>
__device__ __forceinline__ void to_lds(T* dst, const T* src) {
  static_assert(sizeof(T) % sizeof(uint4) == 0, "copied as 16-byte units");
  const uint4* const s = reinterpret_cast<const uint4*>(src);
  uint4* const d = reinterpret_cast<uint4*>(dst);
  for (int u = (int)threadIdx.x; u < (int)(sizeof(T) / sizeof(uint4)); u += SDC_ROWMLP_BLOCK) d[u] = s[u];
}

// A wavefront's rows row0 .. row0 + 15 (n_rows in all, `stride` floats apart): a dword of a row at or past n_rows is not loaded (0)
__device__ __forceinline__ int rows_that_exist(const long long row0, const long long n_rows) {
  const long long left = n_rows - row0;
  return left >= SDC_ROWMLP_ROWS ? SDC_ROWMLP_ROWS : (left > 0 ? (int)left : 0);
}
template <int IN>
__device__ __forceinline__ void fetch(float (&v)[TILE_LOADS<IN>], const float* obs, const long long stride, const long long row0,
                                      const long long n_rows, const int lane) {
  const int valid = rows_that_exist(row0, n_rows);
#pragma unroll
  for (int j = 0; j < TILE_LOADS<IN>; j++) {
    const int u = lane + 64 * j;
    const int r = u / IN, k = u - r * IN;
    v[j] = 0.0f;
    if (r < valid) v[j] = obs[(row0 + r) * stride + k];      // (r < valid <= 16 implies u < 16 IN)
  }
}

// a workgroup's LDS: the network, and a tile per wavefront
template <class DEV, int IN>
struct alignas(16) Lds {      // (16-byte aligned: the A operands and the per-unit vectors are read as 16-byte units)
  DEV net;
  float tile[SDC_ROWMLP_BLOCK / 64][TILE_DW<IN>];
};

}  // namespace sdc_rowmlp
