// sdc_actor_forward.hpp -- one agent's actor over a wavefront's sixteen rows, the forward that sdc_actor_eval.hip (the logits) and
// sdc_actor_grad.hip (the logits and, on a tape, what its backward reads) share: the mapping and the numerics are sdc_actor_eval.hpp's.
//
// forward_kind<KIND, NoTape> is sdc_actor_evaluate's forward as it always was: the critic's epilogue, nothing kept.  With a Tape the same
// operations in the same order (a row's logits are the same bits) leave behind, per lane (g, e) and in the accumulators' layout
// (register (t, i) = unit 16 t + 4 g + i of row e; s = entry 4 s + g of row e):
//   n0[s], rs0      the feature LayerNorm's normalised entries (x - mean) * rs and its rs (untouched when the LayerNorm is off)
//   da1, da2        the activation's derivative from the forward's own values: tanh' = 1 - h^2, relu' = [z > 0]
//   n1, n2, rs1, rs2   the hidden LayerNorms' normalised values and their rs
//   y2              the second hidden LayerNorm's output: the last layer's input
//   y1t             IN: the wavefront's LDS tile that receives the first hidden LayerNorm's output TRANSPOSED, [unit][row], SDC_AEV_TS
//                   dwords between two units (the operand of dW2 += dZ2 Y1^T; sixteen registers that need not live through layer 2)
// and x[] holds layer 1's input (the feature LayerNorm's output when it is on) on return, as it always did.
#pragma once

#include "sdc_actor_eval_pack.hpp"
#include "sdc_critic.hpp"

namespace sdc_aev {

using sdc_act::f4;

#define SDC_AEV_TS 20      // dwords between two units' sixteen rows in a transposed tile: a lane's four rows are one 16-byte read

struct NoTape {};
struct Tape {
  float n0[SDC_AEV_S1], rs0;
  f4 da1[4], n1[4];
  f4 da2[4], n2[4], y2[4];
  float rs1, rs2;
  float* y1t;
};

// sdc_critic::epilogue with the derivative of the activation, the normalised values and rs kept: the same operations in the same order
template <int KIND>
__device__ __forceinline__ void epilogue_taped(f4 (&acc)[4], const float (&gain)[4][4][4], const float (&bias)[4][4][4], const int g,
                                               f4 (&dact)[4], f4 (&n)[4], float& rs_out) {
  float s1 = 0.0f, s2 = 0.0f;
  const float v0 = sdc_critic::group0(sdc_act::activate<KIND>(acc[0][0]));
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float z = acc[t][i];
      const float a = sdc_act::activate<KIND>(z);
      // relu' = [z > 0] = [a > 0] as arithmetic (a >= 0; the smallest positive a times 2^252 is above one): no lane mask to keep
      if constexpr (KIND == 1) dact[t][i] = fminf((a * 0x1p+126f) * 0x1p+126f, 1.0f);
      else dact[t][i] = 1.0f - a * a;
      const float d = a - v0;
      acc[t][i] = d;
      s1 += d;
      s2 += d * d;
    }
  float sum, sq;
  sdc_critic::all_sum2(s1, s2, sum, sq);
  const float mean = sum * (1.0f / SDC_CRITIC_H);
  const float var = fmaxf(sq * (1.0f / SDC_CRITIC_H) - mean * mean, 0.0f);
  const float rs = __builtin_amdgcn_rsqf(var + 1e-5f);
  rs_out = rs;
  f4 gn[4], bs[4];
  sdc_critic::unit_vector(gn, gain, g);
  sdc_critic::unit_vector(bs, bias, g);
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      n[t][i] = (acc[t][i] - mean) * rs;
      acc[t][i] = n[t][i] * gn[t][i] + bs[t][i];
    }
}

// W: the actor in LDS.  x[s]: lane (g, e) holds entry 4 s + g of row e's observation (0 beyond entry 25, and for a row past the last).
// -> the row's three logits, in every lane of column e.
template <int KIND, class TAPE>
__device__ __forceinline__ void forward_kind(const SdcActorEvalDev* W, float (&x)[SDC_AEV_S1], const int lane, float (&lg)[SDC_AEV_OUT],
                                             TAPE& tape) {
  constexpr bool TAPED = !__is_same(TAPE, NoTape);
  const int g = lane >> 4;
  // feature LayerNorm (observation entries are of order one: one unshifted pass, as sdc_actor.hpp's)
  if (W->flags & 1) {
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int s = 0; s < SDC_AEV_S1; s++) {
      s1 += x[s];
      s2 += x[s] * x[s];
    }
    float sum, sq;
    sdc_critic::all_sum2(s1, s2, sum, sq);
    const float mean = sum * (1.0f / SDC_AEV_IN);
    const float var = fmaxf(sq * (1.0f / SDC_AEV_IN) - mean * mean, 0.0f);
    const float rs = __builtin_amdgcn_rsqf(var + 1e-5f);
    if constexpr (TAPED) {
      tape.rs0 = rs;
#pragma unroll
      for (int s = 0; s < SDC_AEV_S1; s++) {
        tape.n0[s] = (x[s] - mean) * rs;
        x[s] = tape.n0[s] * W->ln0_g[g][s] + W->ln0_b[g][s];
      }
    } else {
#pragma unroll
      for (int s = 0; s < SDC_AEV_S1; s++) x[s] = (x[s] - mean) * rs * W->ln0_g[g][s] + W->ln0_b[g][s];      // (gain and bias 0 beyond entry 25)
    }
  }
  // ---- layer 1: 26 (28) -> 64 ------------------------------------------------------------------------------------------------------
  f4 h[4];
  sdc_critic::unit_vector(h, W->b1, g);
#pragma unroll
  for (int s = 0; s < SDC_AEV_S1; s++) {
    const f4 a = *reinterpret_cast<const f4*>(W->a1[s][lane]);
#pragma unroll
    for (int t = 0; t < 4; t++) h[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], x[s], h[t], 0, 0, 0);
  }
  if constexpr (TAPED) {
    epilogue_taped<KIND>(h, W->ln1_g, W->ln1_b, g, tape.da1, tape.n1, tape.rs1);
    const int e = lane & 15;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int i = 0; i < 4; i++) tape.y1t[(16 * t + 4 * g + i) * SDC_AEV_TS + e] = h[t][i];
  } else {
    sdc_critic::epilogue<KIND>(h, W->ln1_g, W->ln1_b, g);
  }
  // ---- layer 2: 64 -> 64; k-step s = 4 t + i reads register (t, i) of layer 1 ------------------------------------------------------
  f4 acc[4];
  sdc_critic::unit_vector(acc, W->b2, g);
#pragma unroll
  for (int s = 0; s < SDC_AEV_S2; s++) {
    const f4 a = *reinterpret_cast<const f4*>(W->a2[s][lane]);
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], h[s >> 2][s & 3], acc[t], 0, 0, 0);
  }
  if constexpr (TAPED) {
    epilogue_taped<KIND>(acc, W->ln2_g, W->ln2_b, g, tape.da2, tape.n2, tape.rs2);
#pragma unroll
    for (int t = 0; t < 4; t++) tape.y2[t] = acc[t];
  } else {
    sdc_critic::epilogue<KIND>(acc, W->ln2_g, W->ln2_b, g);
  }
  // ---- the logits: 64 -> 3 ---------------------------------------------------------------------------------------------------------
  float v[SDC_AEV_OUT];
#pragma unroll
  for (int c = 0; c < SDC_AEV_OUT; c++) {
    f4 w3[4];
    sdc_critic::unit_vector(w3, W->w3[c], g);
    v[c] = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int i = 0; i < 4; i++) v[c] = fmaf(w3[t][i], acc[t][i], v[c]);
  }
  float t0, t1;
  sdc_critic::all_sum2(v[0], v[1], t0, t1);
  const float t2 = sdc_critic::all_sum(v[2]);
  lg[0] = t0 + W->b3[0];
  lg[1] = t1 + W->b3[1];
  lg[2] = t2 + W->b3[2];
}

}  // namespace sdc_aev
