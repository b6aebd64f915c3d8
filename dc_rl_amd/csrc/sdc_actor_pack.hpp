// sdc_actor_pack.hpp -- one agent's actor as the closed-loop kernels read it (SdcActorDev: device memory, then LDS; the mapping that
// asks for this layout: sdc_actor.hpp), and the pack from torch's layout (sdc_actor_params) into it.  sdc_set_actor (sdc_capi.hip)
// builds it next to SdcActorEvalDev (sdc_actor_eval_pack.hpp) and SdcActorGradDev (sdc_actor_grad_pack.hpp) and uploads the three;
// what is refused about an sdc_actor_params stays sdc_set_actor's (sdc_refusals.hpp).
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (sdc_pack_tables.hpp derives the optimiser
// step's gather table from it; tests/test_optim_abi.py holds that table to this pack's bytes).
#pragma once

#include <cstring>

#include "../../include/sustaindc_hip.h"

#define SDC_ACT_IN SDC_OBS_PAD     // 26
#define SDC_ACT_M1 7               // K-quads of layer 1 (26 inputs padded to 28)
#define SDC_ACT_H 64
#define SDC_ACT_M2 (SDC_ACT_H / 4)
#define SDC_ACT_OUT 3

// one agent's actor as the kernel reads it (device memory, then LDS); filled by sdc_set_actor (sdc_capi.hip)
struct SdcActorDev {
  float ln0_g[32], ln0_b[32];                 // feature LayerNorm over the 26 inputs (entries 26.. unused)
  float w1[SDC_ACT_M1][SDC_ACT_H][4];         // w1[m][j][v] = W1[j][4 m + v]   (W as torch stores it: [out][in]; 0 beyond k = 25)
  float w2[SDC_ACT_M2][SDC_ACT_H][4];         // w2[m][j][v] = W2[j][4 m + v]: one ds_read_b128 per lane = four B operands
  float w3[4][SDC_ACT_H];                     // w3[c][j] = W3[c][j], c < 3
  float b1[SDC_ACT_H], ln1_g[SDC_ACT_H], ln1_b[SDC_ACT_H];
  float b2[SDC_ACT_H], ln2_g[SDC_ACT_H], ln2_b[SDC_ACT_H];
  float b3[4];
  int flags;                                  // bit 0: feature LayerNorm on; bits 1-2: activation (0 tanh, 1 relu)
  int pad[3];
};
static_assert(sizeof(SdcActorDev) % 16 == 0, "copied to LDS as uint4");

// torch's [out][in] rows -> the kernel's k-major layout, four consecutive k per lane
inline void sdc_actor_pack(const sdc_actor_params* p, SdcActorDev* d) {
  SdcActorDev& a = *d;
  std::memset(&a, 0, sizeof(a));
  for (int k = 0; k < SDC_ACT_IN; k++) {
    a.ln0_g[k] = p->ln0_gamma[k];
    a.ln0_b[k] = p->ln0_beta[k];
  }
  for (int j = 0; j < SDC_ACT_H; j++) {
    for (int k = 0; k < SDC_ACT_IN; k++) a.w1[k / 4][j][k & 3] = p->w1[j * SDC_ACT_IN + k];
    for (int k = 0; k < SDC_ACT_H; k++) a.w2[k / 4][j][k & 3] = p->w2[j * SDC_ACT_H + k];
    a.b1[j] = p->b1[j]; a.ln1_g[j] = p->ln1_gamma[j]; a.ln1_b[j] = p->ln1_beta[j];
    a.b2[j] = p->b2[j]; a.ln2_g[j] = p->ln2_gamma[j]; a.ln2_b[j] = p->ln2_beta[j];
    for (int c = 0; c < SDC_ACT_OUT; c++) a.w3[c][j] = p->w3[c * SDC_ACT_H + j];
  }
  for (int c = 0; c < SDC_ACT_OUT; c++) a.b3[c] = p->b3[c];
  a.flags = (p->use_feature_normalization ? 1 : 0) | (p->activation << 1);
}
