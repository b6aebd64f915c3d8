// sdc_value_loss_dev.hpp -- the value loss' device code, once: the pass over the elements with sdc_ppo_terms' fold behind it, for
// sdc_value_loss_kernel (sdc_critic_grad.hip: scale and shift are the launch's arguments) and sdc_value_loss_normed_kernel
// (sdc_minibatch.hip: they are read from the handle's ValueNorm block).  The contract: include/sustaindc_hip.h THE CRITIC'S GRADIENT;
// the launch plan and the address bounds: sdc_critic_grad.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sdc_critic_grad.hpp"

namespace {

static_assert((SDC_PPO_BLOCK & (SDC_PPO_BLOCK - 1)) == 0 && SDC_PPO_BLOCK % 64 == 0, "the tree halves whole wavefronts");

// sdc_ppo_terms' fold, word for word (sdc_actor_eval.hip): four sums, a count, a minimum, a maximum
struct Fold {
  double s[7];
};
__device__ __forceinline__ Fold fold_start() {
  return Fold{{0.0, 0.0, 0.0, 0.0, 0.0, __builtin_huge_val(), -__builtin_huge_val()}};
}
// a takes b: the sums a + b, the minimum b < a ? b : a, the maximum b > a ? b : a
__device__ __forceinline__ void fold_take(Fold& a, const Fold& b) {
#pragma unroll
  for (int q = 0; q < 5; q++) a.s[q] = a.s[q] + b.s[q];
  a.s[5] = b.s[5] < a.s[5] ? b.s[5] : a.s[5];
  a.s[6] = b.s[6] > a.s[6] ? b.s[6] : a.s[6];
}
// the workgroup's SDC_PPO_BLOCK folds halved through LDS into lane 0's (every lane runs every round: the barriers are the workgroup's)
__device__ __forceinline__ void halve(double (&part)[7][SDC_PPO_BLOCK], Fold& f, const int l) {
#pragma unroll
  for (int q = 0; q < 7; q++) part[q][l] = f.s[q];
  __syncthreads();
  for (int half = SDC_PPO_BLOCK / 2; half >= 1; half >>= 1) {
    if (l < half) {
      Fold a, b;
#pragma unroll
      for (int q = 0; q < 7; q++) {
        a.s[q] = part[q][l];
        b.s[q] = part[q][l + half];
      }
      fold_take(a, b);
#pragma unroll
      for (int q = 0; q < 7; q++) part[q][l] = a.s[q];
    }
    __syncthreads();
  }
  if (l == 0) {
#pragma unroll
    for (int q = 0; q < 7; q++) f.s[q] = part[q][0];
  }
}

// l(e) and l'(e): Huber with threshold delta, or e^2 / 2
template <bool HUBER>
__device__ __forceinline__ double loss_of(const double e, const double delta) {
  const double sq = (e * e) / 2.0;
  if (!HUBER) return sq;
  const double a = e < 0.0 ? -e : e;
  return a <= delta ? sq : delta * (a - delta / 2.0);
}
template <bool HUBER>
__device__ __forceinline__ double dloss_of(const double e, const double delta) {
  if (!HUBER) return e;
  const double a = e < 0.0 ? -e : e;
  return a <= delta ? e : (e > 0.0 ? delta : -delta);
}

template <bool HUBER, bool STATS>
__device__ __forceinline__ void value_loss_pass(const SdcValueLoss& P, double (&part)[7][SDC_PPO_BLOCK]) {
  const long long stride = (long long)gridDim.x * SDC_PPO_BLOCK;
  const bool clipped_loss = (P.flags & SDC_VALUE_LOSS_CLIPPED) != 0;
  const double clip = P.clip, delta = P.delta;
  Fold f = fold_start();
  for (long long i = (long long)blockIdx.x * SDC_PPO_BLOCK + threadIdx.x; i < P.n; i += stride) {
    const double u = (double)P.raw[i], vp = (double)P.vp[i], ret = (double)P.ret[i];
    const double t = (ret - P.shift) / P.scale;
    const double d = u - vp;
    const double dc = d < -clip ? -clip : (d > clip ? clip : d);
    const double uc = vp + dc;
    const double eo = t - u, ec = t - uc;
    const double lo = loss_of<HUBER>(eo, delta), lc = loss_of<HUBER>(ec, delta);
    const double go = -dloss_of<HUBER>(eo, delta);
    const double gc = (-clip <= d && d <= clip) ? -dloss_of<HUBER>(ec, delta) : 0.0;
    double Lv = lo, g = go;
    if (clipped_loss) {
      Lv = lo > lc ? lo : lc;
      g = lo > lc ? go : (lo < lc ? gc : 0.5 * go + 0.5 * gc);
    }
    const float lf = (float)Lv;
    if (P.loss) P.loss[i] = lf;
    P.dvalue[i] = (float)(P.coef * g);
    if (STATS) {
      f.s[0] = f.s[0] + (double)lf;
      f.s[1] = f.s[1] + u;
      f.s[2] = f.s[2] + eo;
      f.s[3] = f.s[3] + eo * eo;
      f.s[4] = f.s[4] + (lc > lo ? 1.0 : 0.0);
      f.s[5] = eo < f.s[5] ? eo : f.s[5];
      f.s[6] = eo > f.s[6] ? eo : f.s[6];
    }
  }
  if (STATS) {
    const int l = (int)threadIdx.x;
    halve(part, f, l);
    if (l == 0) {
      double* const out = P.part + (size_t)blockIdx.x * SDC_PPO_STATS;
#pragma unroll
      for (int q = 0; q < 7; q++) out[q] = f.s[q];
      out[7] = 0.0;
    }
  }
}

}  // namespace
