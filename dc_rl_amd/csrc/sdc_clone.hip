// sdc_clone.hip -- sdc_clone_kernel: env dst[k] becomes a copy of env src[k] (sdc_clone_envs, sdc_capi.hip).
//
// A bandwidth kernel: ~145 KB per pair at 672-step episodes (ring 40 KB, feature rows 86 KB, weather windows 11 KB, queue table
// 5.5 KB, the rest ~2 KB), ~185 KB with the ring's slot-major mirror.  One launch, three block ranges (sdc_clone.hpp): A the
// env-major rows, B the step-major feature rows, C the slot-major mirrors.  Every write goes to a dst row and every read comes
// from a src row; the host refuses a dst that is also a src or appears twice, so no two lanes write the same byte and no lane
// reads a byte another lane writes -- except H_PEND of a src header, which range A clears while other workgroups may read it
// (the copy writes zeros to the dst's H_PEND whatever it read there).
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_clone.hpp"

namespace {

// (a clang vector, not HIP's uint4: an array of HIP's vector struct is not promoted to registers -- range B's eight loads went
// through scratch memory)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// where unit u of a class lies: the last segment whose first unit is <= u.  The scan is unrolled over the table's capacity, so every
// segment is read at a constant index (a runtime index into the by-value plan would put the plan in scratch memory)
template <int CAP>
__device__ __forceinline__ void unit_addr(const SdcCloneSeg (&T)[CAP], const int n_segs, const unsigned u, const size_t src, const size_t dst,
                                          const unsigned char*& from, unsigned char*& to, unsigned& j, int& seg) {
  unsigned char* base = T[0].base;
  unsigned pitch = T[0].pitch, first = 0;
  seg = 0;
#pragma unroll
  for (int i = 1; i < CAP; i++)
    if (i < n_segs && T[i].first <= u) {
      base = T[i].base;
      pitch = T[i].pitch;
      first = T[i].first;
      seg = i;
    }
  from = base + src * pitch;
  to = base + dst * pitch;
  j = u - first;
}

// header dwords H_PEND .. H_PEND + 3: a dst starts with no deferred re-centring in flight (its windows are src's, valid as they are;
// a request stamped for src -- or for dst's former state -- carries that env's index in its result, which dst must not take over)
__device__ __forceinline__ u32x4 clear_pend(u32x4 v, const unsigned unit) {
  static_assert(H_PEND % 4 == 2, "H_PEND .. H_PEND + 3 are the last two dwords of one 16-byte unit and the first two of the next");
  if (unit == H_PEND / 4) { v.z = 0u; v.w = 0u; }
  if (unit == H_PEND / 4 + 1) { v.x = 0u; v.y = 0u; }
  return v;
}

__device__ __forceinline__ void range_a(const SdcClonePlan& P, const int b, const int tid) {
  const int k = b / P.bpp, part = b - k * P.bpp;
  const int2 pr = P.pairs[k];
  const size_t src = (size_t)pr.x, dst = (size_t)pr.y;
  const unsigned stride = (unsigned)P.bpp * SDC_CLONE_BLOCK;
  // 16-byte units: SDC_CLONE_UNROLL loads in flight per lane before the stores
#pragma unroll 1
  for (unsigned u0 = (unsigned)part * SDC_CLONE_BLOCK + tid; u0 < P.wide_units; u0 += SDC_CLONE_UNROLL * stride) {
    u32x4 v[SDC_CLONE_UNROLL];
    u32x4* to[SDC_CLONE_UNROLL];
    unsigned jj[SDC_CLONE_UNROLL];
    int seg[SDC_CLONE_UNROLL];
#pragma unroll
    for (int i = 0; i < SDC_CLONE_UNROLL; i++) {
      const unsigned u = min(u0 + i * stride, P.wide_units - 1);     // (past the end: the last unit again, copied twice)
      const unsigned char* f;
      unsigned char* t;
      unit_addr(P.wide, P.n_wide, u, src, dst, f, t, jj[i], seg[i]);
      v[i] = reinterpret_cast<const u32x4*>(f)[jj[i]];
      to[i] = reinterpret_cast<u32x4*>(t) + jj[i];
    }
#pragma unroll
    for (int i = 0; i < SDC_CLONE_UNROLL; i++) *to[i] = seg[i] == P.hdr_wide ? clear_pend(v[i], jj[i]) : v[i];
  }
  // dword units (rows whose length or alignment is not a multiple of 16 bytes: the observation rows)
#pragma unroll 1
  for (unsigned u = (unsigned)part * SDC_CLONE_BLOCK + tid; u < P.narrow_units; u += stride) {
    const unsigned char* f;
    unsigned char* t;
    unsigned j;
    int seg;
    unit_addr(P.narrow, P.n_narrow, u, src, dst, f, t, j, seg);
    reinterpret_cast<unsigned*>(t)[j] = reinterpret_cast<const unsigned*>(f)[j];
  }
  // ... and src itself: a request in flight for src would be taken over by src alone, and the two would part in window placement
  if (part == 0 && tid < 4) reinterpret_cast<unsigned*>(P.wide[P.hdr_wide].base + src * P.wide[P.hdr_wide].pitch)[H_PEND + tid] = 0u;
}

__device__ __forceinline__ void range_b(const SdcClonePlan& P, const int b, const int tid) {
  const int grp = b % P.feat_pair_groups, rows0 = (b / P.feat_pair_groups) * SDC_CLONE_FEAT_ROWS;
  const int k = grp * (SDC_CLONE_BLOCK / 8) + tid / 8, q = tid & 7;     // pair, 16-byte quarter-line of its 128-byte row
  if (k >= P.n) return;
  const int2 pr = P.pairs[k];
  constexpr int Q = SDC_FEAT_ROW / 4;      // 16-byte units per feature row
  static_assert(Q == 8, "eight lanes per 128-byte feature row");
  const size_t rs = (size_t)P.n_envs * Q;  // units per step
  const u32x4* from = reinterpret_cast<const u32x4*>(P.feat) + (size_t)pr.x * Q + q;
  u32x4* to = reinterpret_cast<u32x4*>(P.feat) + (size_t)pr.y * Q + q;
  // (the last workgroup's rows past the end are clamped to the last row, which its lane then copies more than once: no branches
  // between the loads and the stores, so the eight loads stay in flight together)
  u32x4 v[SDC_CLONE_FEAT_ROWS];
#pragma unroll
  for (int i = 0; i < SDC_CLONE_FEAT_ROWS; i++) v[i] = from[(size_t)min(rows0 + i, P.feat_rows - 1) * rs];
#pragma unroll
  for (int i = 0; i < SDC_CLONE_FEAT_ROWS; i++) to[(size_t)min(rows0 + i, P.feat_rows - 1) * rs] = v[i];
}

__device__ __forceinline__ void range_c(const SdcClonePlan& P, const int b, const int tid) {
  const int grp = b % P.mirror_pair_groups, rows0 = (b / P.mirror_pair_groups) * SDC_CLONE_MIRROR_ROWS;
  const int k = grp * SDC_CLONE_BLOCK + tid;
  if (k >= P.n) return;
  const int2 pr = P.pairs[k];
  const size_t rs = (size_t)P.n_envs;
  unsigned v[SDC_CLONE_MIRROR_ROWS];      // (rows past the end clamped as in range_b)
#pragma unroll
  for (int i = 0; i < SDC_CLONE_MIRROR_ROWS; i++) v[i] = P.mirror[(size_t)min(rows0 + i, P.mirror_rows - 1) * rs + pr.x];
#pragma unroll
  for (int i = 0; i < SDC_CLONE_MIRROR_ROWS; i++) P.mirror[(size_t)min(rows0 + i, P.mirror_rows - 1) * rs + pr.y] = v[i];
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_CLONE_BLOCK) sdc_clone_kernel(SdcClonePlan P) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (b < P.blocks_a)
    range_a(P, b, tid);
  else if (b < P.blocks_a + P.blocks_b)
    range_b(P, b - P.blocks_a, tid);
  else
    range_c(P, b - P.blocks_a - P.blocks_b, tid);
}

// the grid of a plan: range A, then B, then C
hipError_t sdc_clone_launch(const SdcClonePlan& P, hipStream_t st) {
  const int blocks_c = P.mirror ? P.mirror_pair_groups * ((P.mirror_rows + SDC_CLONE_MIRROR_ROWS - 1) / SDC_CLONE_MIRROR_ROWS) : 0;
  hipLaunchKernelGGL(sdc_clone_kernel, dim3(P.blocks_a + P.blocks_b + blocks_c), dim3(SDC_CLONE_BLOCK), 0, st, P);
  return hipGetLastError();
}
