// sdc_critic_grad_pack.hpp -- the TRANSPOSED weights of the critic as sdc_critic_grad_kernel's backward reads them (SdcCriticGradDev:
// device memory, then LDS), and the pack from torch's layout (sdc_critic_params) into it.  sdc_set_critic (sdc_capi.hip) builds it next
// to SdcCriticDev (sdc_critic_pack.hpp, whose bytes stay what they were) and uploads both.
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_critic_grad_abi.py builds it into a
// small program, un-permutes what it packed and holds it to the input bit for bit).
//
// THE LAYOUT is sdc_actor_grad_pack.hpp's, with 29 inputs for 26: the backward's two products that move no data take a layer's
// pre-activation gradient dZ as it stands in the accumulators -- register (t, i) of lane l = (g = l >> 4, e = l & 15) is unit
// 16 t + 4 g + i of row e -- as the B operand of k-step s = 4 t + i of dY^T = W^T dZ^T, its k index 4 s + g standing for unit
// sdc_rowmlp_unit_of_k(4 s + g).  The A operand holds W^T with its columns numbered so:
//   a2t[s][l][t'] = W2[unit_of_k(4 s + (l >> 4))][16 t' + (l & 15)]          dY1: register (t', r) = unit 16 t' + 4 g + r, layer 1's own layout
//   a1t[s][l][t'] = W1[unit_of_k(4 s + (l >> 4))][entry(t', l & 15)]         t' = 0, 1; entry(t', i) = 16 t' + 4 (i & 3) + (i >> 2), 0 for
//                                                                            entries >= 29
// so that register (t', r) of dX in lane (g, e) is entry 4 (4 t' + r) + g of row e: share_obs' own layout (x[s] = entry 4 s + g,
// s = 4 t' + r), where the feature LayerNorm's normalised entries wait.
#pragma once

#include <cstddef>
#include <cstring>

#include "../../include/sustaindc_hip.h"
#include "sdc_critic_pack.hpp"

struct SdcCriticGradDev {
  float a2t[SDC_ROWMLP_S2][64][4];
  float a1t[SDC_ROWMLP_S2][64][2];
};
static_assert(sizeof(SdcCriticGradDev) % 16 == 0, "copied to LDS as 16-byte units");

// the float members of sdc_critic_params from ln0_g to b3, in declaration order: what sdc_critic_backward's `grads` holds (scale and
// shift are no parameters)
static_assert(SDC_CRITIC_N_PARAMS == offsetof(sdc_critic_params, scale) / 4, "every float member up to b3, no padding");
static_assert(SDC_CRITIC_N_PARAMS == 2 * 29 + 64 * 29 + 3 * 64 + 64 * 64 + 3 * 64 + 64 + 1, "ln0, w1, b1 ln1, w2, b2 ln2, w3, b3");

// the share_obs entry that row i of tile t' of a1t stands for
inline int sdc_critic_grad_entry(const int tp, const int i) { return 16 * tp + 4 * (i & 3) + (i >> 2); }

// torch's layout ([out][in] rows) -> the backward's
inline void sdc_critic_grad_pack(const sdc_critic_params* p, SdcCriticGradDev* d) {
  std::memset(d, 0, sizeof(*d));
  for (int s = 0; s < SDC_ROWMLP_S2; s++)
    for (int l = 0; l < 64; l++) {
      const int g = l >> 4, e = l & 15;
      const int unit = sdc_rowmlp_unit_of_k(4 * s + g);
      for (int t = 0; t < 4; t++) d->a2t[s][l][t] = p->w2[unit * SDC_ROWMLP_H + 16 * t + e];
      for (int t = 0; t < 2; t++) {
        const int k = sdc_critic_grad_entry(t, e);
        d->a1t[s][l][t] = k < SDC_CRITIC_IN ? p->w1[unit * SDC_CRITIC_IN + k] : 0.0f;
      }
    }
}
