// sdc_actor_grad_pack.hpp -- the TRANSPOSED weights of one agent's actor as sdc_actor_grad_kernel's backward reads them
// (SdcActorGradDev: the row networks' SdcRowMlpGradDev with 26 inputs; the layout and the pack: sdc_rowmlp_grad_pack.hpp).
// sdc_set_actor (sdc_capi.hip) builds it next to SdcActorEvalDev (sdc_actor_eval_pack.hpp) and uploads both.
//
// Plain C++17: no HIP, no sdc_handle, no device calls -- a host compiler alone builds it (tests/test_actor_grad_abi.py).
#pragma once

#include <cstddef>

#include "../../include/sustaindc_hip.h"
#include "sdc_actor_eval_pack.hpp"
#include "sdc_rowmlp_grad_pack.hpp"

using SdcActorGradDev = SdcRowMlpGradDev;

// the float members of sdc_actor_params, in declaration order: what sdc_actor_backward's `grads` holds
static_assert(SDC_ACTOR_N_PARAMS * sizeof(float) == offsetof(sdc_actor_params, use_feature_normalization), "every float member, no padding");
static_assert(SDC_ACTOR_N_PARAMS == 2 * 26 + 64 * 26 + 3 * 64 + 64 * 64 + 3 * 64 + 3 * 64 + 3, "ln0, w1, b1 ln1, w2, b2 ln2, w3, b3");

inline void sdc_actor_grad_pack(const sdc_actor_params* p, SdcActorGradDev* d) { sdc_rowmlp_grad_pack<SDC_AEV_IN>(p->w1, p->w2, d); }
