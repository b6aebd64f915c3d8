// sdc_critic_grad_pack.hpp -- the TRANSPOSED weights of the critic as sdc_critic_grad_kernel's backward reads them (SdcCriticGradDev:
// the row networks' SdcRowMlpGradDev with 29 inputs; the layout and the pack: sdc_rowmlp_grad_pack.hpp).  sdc_set_critic
// (sdc_capi.hip) builds it next to SdcCriticDev (sdc_critic_pack.hpp, whose bytes stay what they were) and uploads both.
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_critic_grad_abi.py).
#pragma once

#include <cstddef>

#include "../../include/sustaindc_hip.h"
#include "sdc_critic_pack.hpp"
#include "sdc_rowmlp_grad_pack.hpp"

using SdcCriticGradDev = SdcRowMlpGradDev;

// the float members of sdc_critic_params from ln0_g to b3, in declaration order: what sdc_critic_backward's `grads` holds (scale and
// shift are no parameters)
static_assert(SDC_CRITIC_N_PARAMS == offsetof(sdc_critic_params, scale) / 4, "every float member up to b3, no padding");
static_assert(SDC_CRITIC_N_PARAMS == 2 * 29 + 64 * 29 + 3 * 64 + 64 * 64 + 3 * 64 + 64 + 1, "ln0, w1, b1 ln1, w2, b2 ln2, w3, b3");

inline void sdc_critic_grad_pack(const sdc_critic_params* p, SdcCriticGradDev* d) { sdc_rowmlp_grad_pack<SDC_CRITIC_IN>(p->w1, p->w2, d); }
