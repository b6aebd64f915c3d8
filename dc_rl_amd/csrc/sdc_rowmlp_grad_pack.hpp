// sdc_rowmlp_grad_pack.hpp -- the TRANSPOSED weights of a row network (sdc_rowmlp.hpp: the critic, the stored-row actors) as the shared
// backward (sdc_rowmlp_grad.hpp) reads them (SdcRowMlpGradDev: device memory, then LDS), and the pack from torch's layout into it.
// sdc_actor_grad_pack.hpp and sdc_critic_grad_pack.hpp name it for their network; sdc_set_actor / sdc_set_critic (sdc_capi.hip) build it
// next to the forward's pack and upload both.
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_actor_grad_abi.py and
// tests/test_critic_grad_abi.py build it into small programs, un-permute what it packed and hold it to the input bit for bit).
//
// THE LAYOUT follows the backward's two products that move no data.  The forward leaves a layer's pre-activation gradient dZ in the
// accumulators' layout -- register (t, i) of lane l = (g = l >> 4, e = l & 15) is unit 16 t + 4 g + i of row e --, and that register IS
// the B operand of k-step s = 4 t + i of the transposed product dY^T = W^T dZ^T, its k index 4 s + g standing for unit
// sdc_rowmlp_unit_of_k(4 s + g) (sdc_rowmlp_pack.hpp).  The A operand holds W^T with its columns numbered so:
//   a2t[s][l][t'] = W2[unit_of_k(4 s + (l >> 4))][16 t' + (l & 15)]          dY1: register (t', r) = unit 16 t' + 4 g + r, layer 1's own layout
//   a1t[s][l][t'] = W1[unit_of_k(4 s + (l >> 4))][entry(t', l & 15)]         t' = 0, 1; entry(t', i) = 16 t' + 4 (i & 3) + (i >> 2), 0 for
//                                                                            entries >= IN (26: the actors, 29: the critic)
// The rows of a1t are numbered so that register (t', r) of dX in lane (g, e) is entry 16 t' + 4 r + g = 4 (4 t' + r) + g of row e: the
// input's own layout (x[s] = entry 4 s + g, s = 4 t' + r), where the feature LayerNorm's normalised entries wait.
#pragma once

#include <cstring>

#include "sdc_rowmlp_pack.hpp"

struct SdcRowMlpGradDev {
  float a2t[SDC_ROWMLP_S2][64][4];
  float a1t[SDC_ROWMLP_S2][64][2];
};
static_assert(sizeof(SdcRowMlpGradDev) % 16 == 0, "copied to LDS as 16-byte units");

// the input entry that row i of tile t' of a1t stands for
inline int sdc_rowmlp_grad_entry(const int tp, const int i) { return 16 * tp + 4 * (i & 3) + (i >> 2); }

// torch's layout ([out][in] rows: w1 [64][IN], w2 [64][64]) -> the backward's
template <int IN>
inline void sdc_rowmlp_grad_pack(const float* w1, const float* w2, SdcRowMlpGradDev* d) {
  std::memset(d, 0, sizeof(*d));
  for (int s = 0; s < SDC_ROWMLP_S2; s++)
    for (int l = 0; l < 64; l++) {
      const int g = l >> 4, e = l & 15;
      const int unit = sdc_rowmlp_unit_of_k(4 * s + g);
      for (int t = 0; t < 4; t++) d->a2t[s][l][t] = w2[unit * SDC_ROWMLP_H + 16 * t + e];
      for (int t = 0; t < 2; t++) {
        const int k = sdc_rowmlp_grad_entry(t, e);
        d->a1t[s][l][t] = k < IN ? w1[unit * IN + k] : 0.0f;
      }
    }
}
