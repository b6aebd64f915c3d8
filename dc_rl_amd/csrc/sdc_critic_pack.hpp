// sdc_critic_pack.hpp -- the critic as the kernels read it (SdcCriticDev: device memory, then LDS), what sdc_set_critic refuses about
// an sdc_critic_params, and the pack from torch's layout into the device layout.  sdc_capi.hip calls these and uploads the result.
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_critic_abi.py builds it into a small
// program, un-permutes what it packed and holds it to the input bit for bit).
//
// The trunk (29 inputs in 8 k-steps) and its layout: sdc_rowmlp_pack.hpp.  The head: w3 a per-unit vector, value = (w3 . h + b3) * scale
// + shift.
#pragma once

#include <cmath>
#include <cstddef>

#include "../../include/sustaindc_hip.h"
#include "sdc_rowmlp_pack.hpp"

#define SDC_CRITIC_IN SDC_SHARE_OBS_DIM     // 29
#define SDC_CRITIC_S1 8                     // k-steps of layer 1 (29 inputs padded to 32)

struct SdcCriticDev {
  float a1[SDC_CRITIC_S1][64][4];
  float a2[SDC_ROWMLP_S2][64][4];
  float ln0_g[4][8], ln0_b[4][8];
  float b1[4][4][4], ln1_g[4][4][4], ln1_b[4][4][4];
  float b2[4][4][4], ln2_g[4][4][4], ln2_b[4][4][4];
  float w3[4][4][4];
  float b3, scale, shift;                   // value = (w3 . h + b3) * scale + shift
  int flags;                                // bit 0: feature LayerNorm on; bits 1-2: activation (0 tanh, 1 relu)
};
static_assert(sizeof(SdcCriticDev) % 16 == 0, "copied to LDS as 16-byte units");
static_assert(sizeof(SdcCriticDev) == 26640 && offsetof(SdcCriticDev, w3) == 26368, "the bytes the tests and the NumPy references read");

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
  sdc_rowmlp_pack_trunk<SDC_CRITIC_IN, SDC_CRITIC_S1>({p->ln0_g, p->ln0_b, p->w1, p->b1, p->ln1_g, p->ln1_b, p->w2, p->b2, p->ln2_g, p->ln2_b}, d);
  sdc_rowmlp_pack_units(d->w3, p->w3);
  d->b3 = p->b3;
  d->scale = p->scale;
  d->shift = p->shift;
  d->flags = p->flags;
}
