// sdc_actor_forward.hpp -- one agent's actor over a wavefront's sixteen rows, the forward that sdc_actor_eval.hip (the logits) and
// sdc_actor_grad.hip (the logits and, on a tape, what its backward reads) share: sdc_rowmlp.hpp's trunk with IN = 26 in S1 = 7 k-steps
// (the mapping, the numerics and what a tape holds are written there), and the head: three logits.
#pragma once

#include "sdc_actor_eval_pack.hpp"
#include "sdc_rowmlp.hpp"

namespace sdc_aev {

using Tape = sdc_rowmlp::Tape<SDC_AEV_S1>;

// W: the actor in LDS.  x[s]: lane (g, e) holds entry 4 s + g of row e's observation (0 beyond entry 25, and for a row past the last).
// -> the row's three logits, in every lane of column e: three fmaf chains over the lane's 16 registers in the order (t, i), then the sums
// across the four lane groups.  TAPE: sdc_rowmlp::NoTape (sdc_actor_evaluate: nothing kept) or Tape.
template <int KIND, class TAPE>
__device__ __forceinline__ void forward_kind(const SdcActorEvalDev* W, float (&x)[SDC_AEV_S1], const int lane, float (&lg)[SDC_AEV_OUT],
                                             TAPE& tape) {
  sdc_rowmlp::f4 acc[4];
  sdc_rowmlp::trunk<KIND, SDC_AEV_IN>(W, x, lane, acc, tape);
  float v[SDC_AEV_OUT];
#pragma unroll
  for (int c = 0; c < SDC_AEV_OUT; c++) v[c] = sdc_rowmlp::unit_dot(W->w3[c], acc, lane >> 4);
  float t0, t1;
  sdc_rowmlp::all_sum2(v[0], v[1], t0, t1);
  const float t2 = sdc_rowmlp::all_sum(v[2]);
  lg[0] = t0 + W->b3[0];
  lg[1] = t1 + W->b3[1];
  lg[2] = t2 + W->b3[2];
}

}  // namespace sdc_aev
