// sdc_optim.hpp -- THE ARITHMETIC OF THE OPTIMISER STEP, once: the scalar preparation of one Adam step with gradient-norm clipping
// (sdc_adam_prepare), the step per element (sdc_adam_element), the fixed-order fp64 sum of squares as one lane forms it
// (sdc_adam_lane_sq) and what the entry points refuse about an sdc_adam and an sdc_optim_state.  The contract: include/sustaindc_hip.h
// THE OPTIMISER STEP.  sdc_optim.hip runs these on the device; sdc_adam_step_host below runs the same functions over host arrays.
//
// No HIP beyond the __host__ __device__ markers, no sdc_handle: hipcc and a plain host compiler both build it (tests/test_optim_abi.py
// builds it into small programs with -ffp-contract=off and holds it to the NumPy restatement tests/optim_ref.py bit for bit).
// Every fp32 line below is ONE operation, so that nothing can be contracted whatever the flags.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/sustaindc_hip.h"

#if defined(__HIPCC__)
#define SDC_OPTIM_HD __host__ __device__
#else
#define SDC_OPTIM_HD
#endif

#define SDC_ADAM_SQ_LANES 256      // lanes of the sum of squares: sdc_actor_grad_sq_kernel's (include/sustaindc_hip.h states the order)

// what a step's elements need: every scalar rounded once to fp32
struct SdcAdamScalars {
  float clip;                      // c
  float weight_decay;
  float one_minus_beta1, beta2, one_minus_beta2;
  float rsq;                       // sqrt(1 - beta2 ** step)
  float eps;
  float step_size;                 // lr / (1 - beta1 ** step)
};

// lane l's part of the sum of squares of g[0 .. n): j = l, l + 256, ... in that order
SDC_OPTIM_HD inline double sdc_adam_lane_sq(const float* g, const int n, const int l) {
  double s = 0.0;
  for (int j = l; j < n; j += SDC_ADAM_SQ_LANES) {
    const double v = (double)g[j];
    const double sq = v * v;
    s = s + sq;
  }
  return s;
}

// Steps 2 to 4 of the contract from S, the sum of squares: false (and skipped += 1, nothing else) when S is not finite; else the state
// block moves on and `k` holds the step's scalars.
SDC_OPTIM_HD inline bool sdc_adam_prepare(const sdc_adam& a, const double S, sdc_optim_state& st, SdcAdamScalars& k) {
  if (!(S - S == 0.0)) {           // (NaN or infinity)
    st.skipped += 1;
    return false;
  }
  const double norm = sqrt(S);
  const double ratio = a.max_grad_norm / (norm + 1e-6);
  const double c = ratio < 1.0 ? ratio : 1.0;
  st.step += 1;
  st.beta1_pow = st.beta1_pow * a.beta1;
  st.beta2_pow = st.beta2_pow * a.beta2;
  k.clip = (float)c;
  k.weight_decay = (float)a.weight_decay;
  k.one_minus_beta1 = (float)(1.0 - a.beta1);
  k.beta2 = (float)a.beta2;
  k.one_minus_beta2 = (float)(1.0 - a.beta2);
  k.rsq = (float)sqrt(1.0 - st.beta2_pow);
  k.eps = (float)a.eps;
  k.step_size = (float)(a.lr / (1.0 - st.beta1_pow));
  return true;
}

// Step 5 of the contract: one element
SDC_OPTIM_HD inline void sdc_adam_element(const SdcAdamScalars& k, const float grad, float& p, float& m, float& v) {
  float g = grad * k.clip;
  if (k.weight_decay != 0.0f) {
    const float wp = k.weight_decay * p;
    g = g + wp;
  }
  const float dm = g - m;
  const float wdm = k.one_minus_beta1 * dm;
  m = m + wdm;
  v = v * k.beta2;
  const float bg = k.one_minus_beta2 * g;
  const float bgg = bg * g;
  v = v + bgg;
  const float root = sqrtf(v);
  const float scaled = root / k.rsq;
  const float denom = scaled + k.eps;
  const float q = m / denom;
  const float upd = k.step_size * q;
  p = p - upd;
}

// the whole step over host arrays, in the device's order (what the stand-alone tests run): `first` leading elements are left alone
// (the ln0 entries of a network whose feature LayerNorm is off).  -> sqrt(S)
inline double sdc_adam_step_host(const sdc_adam& a, const float* g, const int n, const int first, float* p, float* m, float* v,
                                 sdc_optim_state& st) {
  double part[SDC_ADAM_SQ_LANES];
  for (int l = 0; l < SDC_ADAM_SQ_LANES; l++) part[l] = sdc_adam_lane_sq(g, n, l);
  for (int half = SDC_ADAM_SQ_LANES / 2; half >= 1; half >>= 1)
    for (int l = 0; l < half; l++) part[l] = part[l] + part[l + half];
  SdcAdamScalars k;
  if (sdc_adam_prepare(a, part[0], st, k))
    for (int j = first; j < n; j++) sdc_adam_element(k, g[j], p[j], m[j], v[j]);
  return sqrt(part[0]);
}

// ---- what the entry points refuse about their scalars (the texts behind the entry point's "who: "; sdc_refusals.hpp) ---------------
inline const char* sdc_adam_error(const sdc_adam* a) {
  if (!a) return "null sdc_adam";
  if (!std::isfinite(a->lr) || a->lr < 0.0) return "lr must be finite and not negative";
  if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0)) return "beta1 and beta2 must lie in [0, 1)";
  if (!std::isfinite(a->eps) || a->eps < 0.0) return "eps must be finite and not negative";
  if (!std::isfinite(a->weight_decay) || a->weight_decay < 0.0) return "weight_decay must be finite and not negative";
  if (!(a->max_grad_norm > 0.0)) return "max_grad_norm must be above 0 (+infinity: no clipping)";
  return nullptr;
}
inline const char* sdc_optim_state_error(const float* m, const float* v, const sdc_optim_state* st, const int n) {
  if (!m || !v || !st) return "null m, v or state";
  if (st->step < 0) return "step must not be negative";
  if (!(st->beta1_pow > 0.0 && st->beta1_pow <= 1.0) || !(st->beta2_pow > 0.0 && st->beta2_pow <= 1.0))
    return "beta1_pow and beta2_pow must lie in (0, 1]";
  if (st->skipped < 0) return "skipped must not be negative";
  for (int j = 0; j < n; j++)
    if (!std::isfinite(m[j]) || !std::isfinite(v[j]) || v[j] < 0.0f) return "a moment that is not finite, or a negative v";
  return nullptr;
}
