// sdc_philox.hpp -- the counter-based generator of the device-side draws, once: Philox4x32-R (Salmon et al., SC'11; Random123's
// known-answer vectors for R = 7 and R = 10 pin the NumPy restatement, tests/test_reset_ref.py, and the restatement pins this code,
// tests/test_gpu_reset_pin.py).  R = 10 for the per-episode draws, the actor's sampler and the mini-batch permutation; R = 7 -- the
// paper's Crush-resistant minimum with a safety margin -- for the 35 040 normals of a reset's weather walk, whose cost is the
// 2 R quarter-rate 32 x 32 -> 64-bit products per block.
//
// No HIP beyond the __host__ __device__ markers: sdc_device.hpp includes it for the kernels, sdc_minibatch.hpp for the kernels and for a
// plain host compiler.
#pragma once

#if defined(__HIPCC__)
#define SDC_PHILOX_HD __host__ __device__ __forceinline__
#define SDC_PHILOX_UNROLL _Pragma("unroll")
#else
#define SDC_PHILOX_HD inline
#define SDC_PHILOX_UNROLL
#endif

struct Philox4 {
  unsigned x, y, z, w;
};
template <int R>
SDC_PHILOX_HD Philox4 philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  SDC_PHILOX_UNROLL
  for (int r = 0; r < R; r++) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
    const unsigned n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    const unsigned n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}
SDC_PHILOX_HD Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  return philox4x32<10>(c0, c1, c2, c3, k0, k1);
}
