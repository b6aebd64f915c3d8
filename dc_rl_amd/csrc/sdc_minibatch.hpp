// sdc_minibatch.hpp -- THE ARITHMETIC OF A SHUFFLED MINI-BATCH AND OF VALUENORM'S RUNNING UPDATE, once: the keyed permutation of
// 0 .. n-1 (sdc_perm_index), the fixed-order fp64 sums of the returns as one lane forms them (sdc_value_norm_lane_sums), the update of
// the three running values and what scale and shift follow from them (sdc_value_norm_update, sdc_value_norm_derive), and what the
// entry points refuse about an sdc_value_norm and a table of gather segments.  The contract: include/sustaindc_hip.h TRAIN ON THE
// DEVICE.  sdc_minibatch.hip runs these on the device; the *_host functions below run the same functions over host arrays.
//
// No HIP beyond the __host__ __device__ markers, no sdc_handle: hipcc and a plain host compiler both build it (tests/test_train_abi.py
// builds it into small programs with -ffp-contract=off and holds it to the NumPy restatement tests/train_ref.py bit for bit).  Every
// fp32 line below is ONE operation, so that nothing can be contracted whatever the flags.
//
// THE PERMUTATION IS A PSEUDO-RANDOM BIJECTION FOR SHUFFLING ROWS, NOT A UNIFORM DRAW FROM ALL n! PERMUTATIONS: a six-round Feistel
// network over 4^b >= n values, its round function one philox4x32_10 block, walked until it lands below n.  There are at most
// 2^128 keys, and of a key's 4^b-cycle structure only the part below n is seen.  What it is held to: a bijection for every n, and
// position-by-value counts over 4096 streams that a chi-square test does not tell from uniform (four rounds fail that test at n = 12:
// 234 on 121 degrees of freedom against 129 with six).
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/sustaindc_hip.h"
#include "sdc_philox.hpp"

#if defined(__HIPCC__)
#define SDC_MB_HD __host__ __device__
#else
#define SDC_MB_HD
#endif

#define SDC_PERM_ROUNDS 6
#define SDC_PERM_MAX_N 2147483647ll      // 2^31 - 1: the outputs are int32
#define SDC_VN_BLOCK 256                 // lanes per workgroup of both stages of the sums: sdc_ppo_terms' (SDC_PPO_BLOCK)
#define SDC_VN_MAX_BLOCKS 1024           // stage 1's cap (SDC_PPO_MAX_BLOCKS)

// ---- the permutation ---------------------------------------------------------------------------------------------------------------------
struct SdcPermKey {
  unsigned n;                      // 1 .. 2^31 - 1
  unsigned b, mask;                // half the block's width in bits, 2^b - 1
  unsigned seed_lo, seed_hi, stream_lo, stream_hi;
};

// bits = bit length of (n - 1) (0 for n = 1); b = max(1, (bits + 1) / 2): 4^b >= n, and 4^b < 4 n for n >= 2
SDC_MB_HD inline SdcPermKey sdc_perm_key(const long long n, const uint64_t seed, const uint64_t stream_id) {
  unsigned bits = 0;
  for (unsigned long long v = (unsigned long long)(n - 1); v != 0; v >>= 1) bits++;
  const unsigned half = (bits + 1) / 2;
  const unsigned b = half < 1 ? 1 : half;
  return SdcPermKey{(unsigned)n, b, (1u << b) - 1u, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)stream_id, (unsigned)(stream_id >> 32)};
}

// perm[i]: i < n through the Feistel network until the value lies below n again (cycle walking: a bijection of 0 .. 4^b - 1 restricted
// to the cycle structure below n is a bijection of 0 .. n-1; a lane walks fewer than four times on average).  b <= 16: x fits 32 bits.
SDC_MB_HD inline unsigned sdc_perm_index(const unsigned i, const SdcPermKey& k) {
  unsigned x = i;
  do {
    unsigned L = x >> k.b, R = x & k.mask;
    for (unsigned r = 0; r < SDC_PERM_ROUNDS; r++) {
      const unsigned F = philox4x32_10(R, r, k.stream_lo, k.stream_hi, k.seed_lo, k.seed_hi).x & k.mask;
      const unsigned nr = L ^ F;
      L = R;
      R = nr;
    }
    x = (L << k.b) | R;
  } while (x >= k.n);
  return x;
}

inline void sdc_permutation_host(const long long n, const uint64_t seed, const uint64_t stream_id, int32_t* perm) {
  const SdcPermKey k = sdc_perm_key(n, seed, stream_id);
  for (long long i = 0; i < n; i++) perm[i] = (int32_t)sdc_perm_index((unsigned)i, k);
}

// ---- ValueNorm ------------------------------------------------------------------------------------------------------------------------
// the handle's device block: sdc_value_norm's three values and what follows from them
struct SdcValueNormDev {
  float running_mean, running_mean_sq, debiasing_term;
  float scale, shift;              // value * scale + shift denormalises: sqrt(var), mean
};

// stage 1's workgroups for n elements: sdc_ppo_blocks' rule
SDC_MB_HD inline int sdc_value_norm_blocks(const long long n) {
  const long long want = (n + SDC_VN_BLOCK - 1) / SDC_VN_BLOCK;
  return (int)(want < SDC_VN_MAX_BLOCKS ? want : SDC_VN_MAX_BLOCKS);
}

// lane l of workgroup b of B: S1 += (double)x, S2 += (double)(float)(x * x) over i = b * 256 + l + k * 256 * B, k = 0, 1, ... in that order
SDC_MB_HD inline void sdc_value_norm_lane_sums(const float* x, const long long n, const int B, const int b, const int l, double& s1, double& s2) {
  s1 = 0.0;
  s2 = 0.0;
  const long long stride = (long long)B * SDC_VN_BLOCK;
  for (long long i = (long long)b * SDC_VN_BLOCK + l; i < n; i += stride) {
    const float v = x[i];
    const float sq = v * v;
    s1 = s1 + (double)v;
    s2 = s2 + (double)sq;
  }
}

// harl/common/valuenorm.py running_mean_var and denormalize, fp32: the debiasing term clamped at 1e-5, the variance at 1e-2
// (dc_rl_amd.engine.value_norm_scale_shift is the same lines in NumPy)
SDC_MB_HD inline void sdc_value_norm_derive(SdcValueNormDev& s) {
  const float deb = s.debiasing_term < 1e-5f ? 1e-5f : s.debiasing_term;
  const float mean = s.running_mean / deb;
  const float mean_sq = s.running_mean_sq / deb;
  const float mm = mean * mean;
  const float dv = mean_sq - mm;
  const float var = dv < 1e-2f ? 1e-2f : dv;
  s.scale = sqrtf(var);
  s.shift = mean;
}

// ValueNorm.update (per_element_update False) from the two sums over n values
SDC_MB_HD inline void sdc_value_norm_update(SdcValueNormDev& s, const double S1, const double S2, const long long n, const double beta) {
  const float bm = (float)(S1 / (double)n);
  const float bsq = (float)(S2 / (double)n);
  const float w = (float)beta;
  const float omw = (float)(1.0 - beta);
  const float a1 = s.running_mean * w;
  const float b1 = bm * omw;
  s.running_mean = a1 + b1;
  const float a2 = s.running_mean_sq * w;
  const float b2 = bsq * omw;
  s.running_mean_sq = a2 + b2;
  const float a3 = s.debiasing_term * w;
  s.debiasing_term = a3 + omw;
  sdc_value_norm_derive(s);
}

// the tree of both stages over one workgroup's lanes: for half = 128, 64, .. 1 lane l < half takes lane l + half
inline void sdc_value_norm_halve_host(double (&p)[2][SDC_VN_BLOCK]) {
  for (int half = SDC_VN_BLOCK / 2; half >= 1; half >>= 1)
    for (int l = 0; l < half; l++)
      for (int q = 0; q < 2; q++) p[q][l] = p[q][l] + p[q][l + half];
}
// the whole update over a host array, in the device's order (what the stand-alone tests run)
inline void sdc_value_norm_update_host(SdcValueNormDev& s, const float* x, const long long n, const double beta) {
  const int B = sdc_value_norm_blocks(n);
  double lane[2][SDC_VN_BLOCK], fold[2][SDC_VN_BLOCK];
  for (int q = 0; q < 2; q++)
    for (int l = 0; l < SDC_VN_BLOCK; l++) fold[q][l] = 0.0;
  for (int b = 0; b < B; b++) {      // (stage 2's lane b % 256 takes partial b: in rising b, as the device's lane does)
    for (int l = 0; l < SDC_VN_BLOCK; l++) sdc_value_norm_lane_sums(x, n, B, b, l, lane[0][l], lane[1][l]);
    sdc_value_norm_halve_host(lane);
    for (int q = 0; q < 2; q++) fold[q][b % SDC_VN_BLOCK] = fold[q][b % SDC_VN_BLOCK] + lane[q][0];
  }
  sdc_value_norm_halve_host(fold);
  sdc_value_norm_update(s, fold[0][0], fold[1][0], n, beta);
}

// ---- what the entry points refuse (the texts behind the entry point's "who: "; sdc_refusals.hpp) -----------------------------------------
inline const char* sdc_value_norm_error(const sdc_value_norm* st) {
  if (!std::isfinite(st->running_mean) || !std::isfinite(st->running_mean_sq) || !std::isfinite(st->debiasing_term))
    return "an entry that is not finite";
  if (st->running_mean_sq < 0.0f || st->debiasing_term < 0.0f) return "running_mean_sq and debiasing_term must not be negative";
  SdcValueNormDev d{st->running_mean, st->running_mean_sq, st->debiasing_term, 0.0f, 0.0f};
  sdc_value_norm_derive(d);
  if (!std::isfinite(d.scale) || !std::isfinite(d.shift)) return "the debiased mean or variance is not finite";
  return nullptr;
}
// a gather segment: -1 accepted, else which rule it breaks (0 a null array, 1 alignment, 2 n_dwords, 3 a stride)
inline int sdc_gather_segment_error(const sdc_gather_segment& g) {
  if (!g.src || !g.dst) return 0;
  if (((reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.dst)) & 3u) != 0) return 1;
  if (g.n_dwords < 1) return 2;
  if (g.src_stride < g.n_dwords || g.dst_stride < g.n_dwords) return 3;
  return -1;
}
