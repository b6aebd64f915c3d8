// sdc_critic_pack.hpp -- the critic as the kernels read it (SdcCriticDev: device memory, then LDS), what sdc_set_critic refuses about
// an sdc_critic_params, and the pack from torch's layout into the device layout.  sdc_capi.hip calls these and uploads the result.
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_critic_abi.py builds it into a small
// program, un-permutes what it packed and holds it to the input bit for bit).
//
// THE LAYOUT follows the kernels' mapping (sdc_critic.hpp): a wavefront takes 16 rows, lane l = (g = l >> 4, e = l & 15) works on row e,
// and a hidden layer is the transposed product H^T = W X^T on v_mfma_f32_16x16x4_f32 -- the 64 units on the A side in four tiles t of 16,
// the rows on the B side.  Accumulator register i of tile t in lane group g then holds unit 16 t + 4 g + i of row e.
//   a1[s][l][t] = W1[16 t + (l & 15)][4 s + (l >> 4)]          the A operand of layer 1's k-step s (k = 4 s + g; 0 for k >= 29): one
//                                                              16-byte LDS read per lane and k-step serves the four tiles
//   a2[s][l][t] = W2[16 t + (l & 15)][unit_of_k(4 s + (l >> 4))]
// Layer 2's k-step s = 4 t' + i' takes as its B operand accumulator register (t', i') of layer 1 as it stands -- the lanes of group g
// hold unit 16 t' + 4 g + i' there, so k = 4 s + g = 16 t' + 4 i' + g of layer 2 IS that unit: W2's columns are renumbered
// (sdc_critic_unit_of_k swaps the two 2-bit fields), nothing moves between the layers.
//   v[g][t][i]  = v[16 t + 4 g + i]     every per-unit vector (b1, ln1_g, ln1_b, b2, ln2_g, ln2_b, w3): a lane reads its 16 entries as
//                                       four 16-byte units
//   ln0_g[g][s] = gamma0[4 s + g]       the feature LayerNorm's, as the lane holds the row's entries (0 beyond entry 28)
// A LayerNorm is symmetric in the units and the last layer is a sum over them: the renumbering never shows outside this file.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstring>

#include "../../include/sustaindc_hip.h"

#define SDC_CRITIC_IN SDC_SHARE_OBS_DIM     // 29
#define SDC_CRITIC_S1 8                     // k-steps of layer 1 (29 inputs padded to 32)
#define SDC_CRITIC_H 64
#define SDC_CRITIC_S2 (SDC_CRITIC_H / 4)    // k-steps of layer 2
#define SDC_CRITIC_ROWS 16                  // rows per wavefront

struct SdcCriticDev {
  float a1[SDC_CRITIC_S1][64][4];
  float a2[SDC_CRITIC_S2][64][4];
  float ln0_g[4][SDC_CRITIC_S1], ln0_b[4][SDC_CRITIC_S1];
  float b1[4][4][4], ln1_g[4][4][4], ln1_b[4][4][4];
  float b2[4][4][4], ln2_g[4][4][4], ln2_b[4][4][4];
  float w3[4][4][4];
  float b3, scale, shift;                   // value = (w3 . h + b3) * scale + shift
  int flags;                                // bit 0: feature LayerNorm on; bits 1-2: activation (0 tanh, 1 relu)
};
static_assert(sizeof(SdcCriticDev) % 16 == 0, "copied to LDS as 16-byte units");

// the hidden unit that layer 2's k index stands for: k = 16 t + 4 i + g <-> unit 16 t + 4 g + i
inline int sdc_critic_unit_of_k(const int k) { return (k & 0x30) | ((k & 3) << 2) | ((k >> 2) & 3); }

// what sdc_set_critic refuses about the parameters -> nullptr, or the reason
inline const char* sdc_critic_params_error(const sdc_critic_params* p) {
  const float* const f = reinterpret_cast<const float*>(p);
  const size_t n_floats = offsetof(sdc_critic_params, flags) / sizeof(float);
  for (size_t j = 0; j < n_floats; j++)
    if (!std::isfinite(f[j])) return "an entry that is not finite";
  if (!(p->scale > 0.0f)) return "scale must be positive";
  if (p->flags < 0 || (p->flags >> 3) != 0) return "unknown flag bits (bit 0: feature LayerNorm, bits 1-2: activation)";
  if (((p->flags >> 1) & 3) > 1) return "unknown activation code (0 tanh, 1 relu)";
  return nullptr;
}

// torch's layout ([out][in] rows) -> the kernels'
inline void sdc_critic_pack(const sdc_critic_params* p, SdcCriticDev* d) {
  std::memset(d, 0, sizeof(*d));
  for (int l = 0; l < 64; l++) {
    const int g = l >> 4, e = l & 15;
    for (int t = 0; t < 4; t++) {
      const int unit = 16 * t + e;
      for (int s = 0; s < SDC_CRITIC_S1; s++) {
        const int k = 4 * s + g;
        d->a1[s][l][t] = k < SDC_CRITIC_IN ? p->w1[unit * SDC_CRITIC_IN + k] : 0.0f;
      }
      for (int s = 0; s < SDC_CRITIC_S2; s++) d->a2[s][l][t] = p->w2[unit * SDC_CRITIC_H + sdc_critic_unit_of_k(4 * s + g)];
    }
  }
  for (int g = 0; g < 4; g++) {
    for (int s = 0; s < SDC_CRITIC_S1; s++) {
      const int k = 4 * s + g;
      d->ln0_g[g][s] = k < SDC_CRITIC_IN ? p->ln0_g[k] : 0.0f;
      d->ln0_b[g][s] = k < SDC_CRITIC_IN ? p->ln0_b[k] : 0.0f;
    }
    for (int t = 0; t < 4; t++)
      for (int i = 0; i < 4; i++) {
        const int unit = 16 * t + 4 * g + i;
        d->b1[g][t][i] = p->b1[unit]; d->ln1_g[g][t][i] = p->ln1_g[unit]; d->ln1_b[g][t][i] = p->ln1_b[unit];
        d->b2[g][t][i] = p->b2[unit]; d->ln2_g[g][t][i] = p->ln2_g[unit]; d->ln2_b[g][t][i] = p->ln2_b[unit];
        d->w3[g][t][i] = p->w3[unit];
      }
  }
  d->b3 = p->b3;
  d->scale = p->scale;
  d->shift = p->shift;
  d->flags = p->flags;
}
