// sdc_actor_eval_pack.hpp -- one agent's actor as sdc_actor_eval_kernel reads it (SdcActorEvalDev: device memory, then LDS), and the
// pack from torch's layout (sdc_actor_params) into it.  sdc_set_actor (sdc_capi.hip) builds it next to the closed loop's SdcActorDev and
// uploads both; what is refused about an sdc_actor_params stays sdc_set_actor's (sdc_refusals.hpp).
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_actor_eval_abi.py builds it into a
// small program, un-permutes what it packed and holds it to the input bit for bit).
//
// THE LAYOUT follows the kernel's mapping (sdc_actor_eval.hpp), which is the critic's (sdc_critic_pack.hpp): a wavefront takes 16 rows,
// lane l = (g = l >> 4, e = l & 15) works on row e, a hidden layer is the transposed product H^T = W X^T on v_mfma_f32_16x16x4_f32 --
// the 64 units on the A side in four tiles t of 16, the rows on the B side; accumulator register i of tile t in lane group g holds unit
// 16 t + 4 g + i of row e.
//   a1[s][l][t] = W1[16 t + (l & 15)][4 s + (l >> 4)]          the A operand of layer 1's k-step s (k = 4 s + g; 0 for k >= 26)
//   a2[s][l][t] = W2[16 t + (l & 15)][unit_of_k(4 s + (l >> 4))]
// Layer 2's k-step s = 4 t' + i' takes accumulator register (t', i') of layer 1 as its B operand as it stands: W2's columns are
// renumbered by sdc_critic_unit_of_k (k = 16 t' + 4 i' + g <-> unit 16 t' + 4 g + i'), nothing moves between the layers.
//   v[g][t][i]     = v[16 t + 4 g + i]        every per-unit vector (b1, ln1_g, ln1_b, b2, ln2_g, ln2_b): four 16-byte units per lane
//   w3[c][g][t][i] = W3[c][16 t + 4 g + i]    the last layer's three rows, each a per-unit vector
//   ln0_g[g][s]    = gamma0[4 s + g]          the feature LayerNorm's, as the lane holds the row's entries (0 beyond entry 25)
// A LayerNorm is symmetric in the units and the last layer is a sum over them: the renumbering never shows outside this file.
#pragma once

#include <cstring>

#include "../../include/sustaindc_hip.h"
#include "sdc_critic_pack.hpp"

#define SDC_AEV_IN 26                       // an agent's zero-padded observation (SDC_OBS_PAD)
#define SDC_AEV_S1 7                        // k-steps of layer 1 (26 inputs padded to 28)
#define SDC_AEV_H 64
#define SDC_AEV_S2 (SDC_AEV_H / 4)          // k-steps of layer 2
#define SDC_AEV_OUT 3
#define SDC_AEV_ROWS 16                     // rows per wavefront

struct SdcActorEvalDev {
  float a1[SDC_AEV_S1][64][4];
  float a2[SDC_AEV_S2][64][4];
  float ln0_g[4][8], ln0_b[4][8];           // (entries s = 7 are padding: 0)
  float b1[4][4][4], ln1_g[4][4][4], ln1_b[4][4][4];
  float b2[4][4][4], ln2_g[4][4][4], ln2_b[4][4][4];
  float w3[SDC_AEV_OUT][4][4][4];
  float b3[4];                              // (entry 3 is padding: 0)
  int flags;                                // bit 0: feature LayerNorm on; bits 1-2: activation (0 tanh, 1 relu) -- SdcActorDev's
  int pad[3];
};
static_assert(sizeof(SdcActorEvalDev) % 16 == 0, "copied to LDS as 16-byte units");
static_assert(SDC_AEV_H == SDC_CRITIC_H, "sdc_critic_unit_of_k numbers 64 units");

// torch's layout ([out][in] rows) -> the kernel's
inline void sdc_actor_eval_pack(const sdc_actor_params* p, SdcActorEvalDev* d) {
  std::memset(d, 0, sizeof(*d));
  for (int l = 0; l < 64; l++) {
    const int g = l >> 4, e = l & 15;
    for (int t = 0; t < 4; t++) {
      const int unit = 16 * t + e;
      for (int s = 0; s < SDC_AEV_S1; s++) {
        const int k = 4 * s + g;
        d->a1[s][l][t] = k < SDC_AEV_IN ? p->w1[unit * SDC_AEV_IN + k] : 0.0f;
      }
      for (int s = 0; s < SDC_AEV_S2; s++) d->a2[s][l][t] = p->w2[unit * SDC_AEV_H + sdc_critic_unit_of_k(4 * s + g)];
    }
  }
  for (int g = 0; g < 4; g++) {
    for (int s = 0; s < SDC_AEV_S1; s++) {
      const int k = 4 * s + g;
      d->ln0_g[g][s] = k < SDC_AEV_IN ? p->ln0_gamma[k] : 0.0f;
      d->ln0_b[g][s] = k < SDC_AEV_IN ? p->ln0_beta[k] : 0.0f;
    }
    for (int t = 0; t < 4; t++)
      for (int i = 0; i < 4; i++) {
        const int unit = 16 * t + 4 * g + i;
        d->b1[g][t][i] = p->b1[unit]; d->ln1_g[g][t][i] = p->ln1_gamma[unit]; d->ln1_b[g][t][i] = p->ln1_beta[unit];
        d->b2[g][t][i] = p->b2[unit]; d->ln2_g[g][t][i] = p->ln2_gamma[unit]; d->ln2_b[g][t][i] = p->ln2_beta[unit];
        for (int c = 0; c < SDC_AEV_OUT; c++) d->w3[c][g][t][i] = p->w3[c * SDC_AEV_H + unit];
      }
  }
  for (int c = 0; c < SDC_AEV_OUT; c++) d->b3[c] = p->b3[c];
  d->flags = (p->use_feature_normalization ? 1 : 0) | (p->activation << 1);
}
