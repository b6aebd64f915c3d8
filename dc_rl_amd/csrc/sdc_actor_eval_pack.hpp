// sdc_actor_eval_pack.hpp -- one agent's actor as sdc_actor_eval_kernel reads it (SdcActorEvalDev: device memory, then LDS), and the
// pack from torch's layout (sdc_actor_params) into it.  sdc_set_actor (sdc_capi.hip) builds it next to the closed loop's SdcActorDev and
// uploads both; what is refused about an sdc_actor_params stays sdc_set_actor's (sdc_refusals.hpp).
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_actor_eval_abi.py builds it into a
// small program, un-permutes what it packed and holds it to the input bit for bit).
//
// The trunk (26 inputs in 7 k-steps) and its layout: sdc_rowmlp_pack.hpp.  The head:
//   w3[c][g][t][i] = W3[c][16 t + 4 g + i]    the last layer's three rows, each a per-unit vector
#pragma once

#include <cstddef>

#include "../../include/sustaindc_hip.h"
#include "sdc_rowmlp_pack.hpp"

#define SDC_AEV_IN 26                       // an agent's zero-padded observation (SDC_OBS_PAD)
#define SDC_AEV_S1 7                        // k-steps of layer 1 (26 inputs padded to 28)
#define SDC_AEV_OUT 3

struct SdcActorEvalDev {
  float a1[SDC_AEV_S1][64][4];
  float a2[SDC_ROWMLP_S2][64][4];
  float ln0_g[4][8], ln0_b[4][8];           // (entries s = 7 are padding: 0)
  float b1[4][4][4], ln1_g[4][4][4], ln1_b[4][4][4];
  float b2[4][4][4], ln2_g[4][4][4], ln2_b[4][4][4];
  float w3[SDC_AEV_OUT][4][4][4];
  float b3[4];                              // (entry 3 is padding: 0)
  int flags;                                // bit 0: feature LayerNorm on; bits 1-2: activation (0 tanh, 1 relu) -- SdcActorDev's
  int pad[3];
};
static_assert(sizeof(SdcActorEvalDev) % 16 == 0, "copied to LDS as 16-byte units");
static_assert(sizeof(SdcActorEvalDev) == 26144 && offsetof(SdcActorEvalDev, w3) == 25344, "the bytes the tests and the NumPy references read");

// torch's layout ([out][in] rows) -> the kernel's
inline void sdc_actor_eval_pack(const sdc_actor_params* p, SdcActorEvalDev* d) {
  sdc_rowmlp_pack_trunk<SDC_AEV_IN, SDC_AEV_S1>(
      {p->ln0_gamma, p->ln0_beta, p->w1, p->b1, p->ln1_gamma, p->ln1_beta, p->w2, p->b2, p->ln2_gamma, p->ln2_beta}, d);
  for (int c = 0; c < SDC_AEV_OUT; c++) {
    sdc_rowmlp_pack_units(d->w3[c], p->w3 + c * SDC_ROWMLP_H);
    d->b3[c] = p->b3[c];
  }
  d->flags = (p->use_feature_normalization ? 1 : 0) | (p->activation << 1);
}
