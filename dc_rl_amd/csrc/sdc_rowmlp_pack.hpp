// sdc_rowmlp_pack.hpp -- the trunk that the critic (SdcCriticDev, sdc_critic_pack.hpp) and the stored-row actors (SdcActorEvalDev,
// sdc_actor_eval_pack.hpp) share, as the kernels of sdc_rowmlp.hpp read it: the layout, and the pack from torch's layout into it.
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_critic_abi.py and
// tests/test_actor_eval_abi.py build its two callers into small programs, un-permute what they packed and hold it to the input bit for bit).
//
// THE LAYOUT follows the kernels' mapping (sdc_rowmlp.hpp): a wavefront takes 16 rows, lane l = (g = l >> 4, e = l & 15) works on row e,
// and a hidden layer is the transposed product H^T = W X^T on v_mfma_f32_16x16x4_f32 -- the 64 units on the A side in four tiles t of 16,
// the rows on the B side.  Accumulator register i of tile t in lane group g then holds unit 16 t + 4 g + i of row e.
//   a1[s][l][t] = W1[16 t + (l & 15)][4 s + (l >> 4)]          the A operand of layer 1's k-step s (k = 4 s + g; 0 for k >= IN): one
//                                                              16-byte LDS read per lane and k-step serves the four tiles
//   a2[s][l][t] = W2[16 t + (l & 15)][unit_of_k(4 s + (l >> 4))]
// Layer 2's k-step s = 4 t' + i' takes as its B operand accumulator register (t', i') of layer 1 as it stands -- the lanes of group g
// hold unit 16 t' + 4 g + i' there, so k = 4 s + g = 16 t' + 4 i' + g of layer 2 IS that unit: W2's columns are renumbered
// (sdc_rowmlp_unit_of_k swaps the two 2-bit fields), nothing moves between the layers.
//   v[g][t][i]  = v[16 t + 4 g + i]     every per-unit vector (b1, ln1_g, ln1_b, b2, ln2_g, ln2_b, a row of the last layer): a lane reads
//                                       its 16 entries as four 16-byte units
//   ln0_g[g][s] = gamma0[4 s + g]       the feature LayerNorm's, as the lane holds the row's entries (0 beyond entry IN - 1)
// A LayerNorm is symmetric in the units and the last layer is a sum over them: the renumbering never shows outside the pack.
//
// A device struct of this trunk starts with the members
//   float a1[S1][64][4], a2[SDC_ROWMLP_S2][64][4], ln0_g[4][8], ln0_b[4][8], b1[4][4][4], ln1_g, ln1_b, b2, ln2_g, ln2_b (each [4][4][4]);
// its head (the last layer, flags: bit 0 feature LayerNorm on, bits 1-2 the activation, 0 tanh, 1 relu) is its own.
#pragma once

#include <cstring>

#define SDC_ROWMLP_H 64                     // hidden units of both layers
#define SDC_ROWMLP_S2 (SDC_ROWMLP_H / 4)    // k-steps of layer 2
#define SDC_ROWMLP_ROWS 16                  // rows per wavefront

// the hidden unit that layer 2's k index stands for: k = 16 t + 4 i + g <-> unit 16 t + 4 g + i
inline int sdc_rowmlp_unit_of_k(const int k) { return (k & 0x30) | ((k & 3) << 2) | ((k >> 2) & 3); }

// a per-unit vector, torch's order -> the lanes'
inline void sdc_rowmlp_pack_units(float (&d)[4][4][4], const float* v) {
  for (int g = 0; g < 4; g++)
    for (int t = 0; t < 4; t++)
      for (int i = 0; i < 4; i++) d[g][t][i] = v[16 * t + 4 * g + i];
}

// the trunk's members of a network in torch's layout ([out][in] rows), in the order the two params structs declare them
struct SdcRowMlpParams {
  const float *ln0_g, *ln0_b, *w1, *b1, *ln1_g, *ln1_b, *w2, *b2, *ln2_g, *ln2_b;
};

// torch's layout -> the kernels': *d is zeroed (its padding with it), then the trunk's members are filled; the head is the caller's
template <int IN, int S1, class DEV>
inline void sdc_rowmlp_pack_trunk(const SdcRowMlpParams& p, DEV* d) {
  static_assert(4 * S1 >= IN && 4 * (S1 - 1) < IN && S1 <= 8, "k-steps of four cover the inputs; ln0 holds eight per lane group");
  std::memset(d, 0, sizeof(*d));
  for (int l = 0; l < 64; l++) {
    const int g = l >> 4, e = l & 15;
    for (int t = 0; t < 4; t++) {
      const int unit = 16 * t + e;
      for (int s = 0; s < S1; s++) {
        const int k = 4 * s + g;
        d->a1[s][l][t] = k < IN ? p.w1[unit * IN + k] : 0.0f;
      }
      for (int s = 0; s < SDC_ROWMLP_S2; s++) d->a2[s][l][t] = p.w2[unit * SDC_ROWMLP_H + sdc_rowmlp_unit_of_k(4 * s + g)];
    }
  }
  for (int g = 0; g < 4; g++)
    for (int s = 0; s < S1; s++) {
      const int k = 4 * s + g;
      d->ln0_g[g][s] = k < IN ? p.ln0_g[k] : 0.0f;
      d->ln0_b[g][s] = k < IN ? p.ln0_b[k] : 0.0f;
    }
  sdc_rowmlp_pack_units(d->b1, p.b1); sdc_rowmlp_pack_units(d->ln1_g, p.ln1_g); sdc_rowmlp_pack_units(d->ln1_b, p.ln1_b);
  sdc_rowmlp_pack_units(d->b2, p.b2); sdc_rowmlp_pack_units(d->ln2_g, p.ln2_g); sdc_rowmlp_pack_units(d->ln2_b, p.ln2_b);
}
