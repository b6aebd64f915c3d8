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
      unsigned char* base;
      unsigned pitch, first;
      seg_find(P.wide, P.n_wide, u, base, pitch, first, seg[i]);
      const unsigned char* const f = base + src * pitch;
      unsigned char* const t = base + dst * pitch;
      jj[i] = u - first;
      v[i] = reinterpret_cast<const u32x4*>(f)[jj[i]];
      to[i] = reinterpret_cast<u32x4*>(t) + jj[i];
    }
#pragma unroll
    for (int i = 0; i < SDC_CLONE_UNROLL; i++) *to[i] = seg[i] == P.hdr_wide ? clear_pend(v[i], jj[i]) : v[i];     // (dst's stamps)
  }
  // dword units (rows whose length or alignment is not a multiple of 16 bytes: the observation rows)
#pragma unroll 1
  for (unsigned u = (unsigned)part * SDC_CLONE_BLOCK + tid; u < P.narrow_units; u += stride) {
    unsigned char* base;
    unsigned pitch, first;
    int seg;
    seg_find(P.narrow, P.n_narrow, u, base, pitch, first, seg);
    const unsigned char* const f = base + src * pitch;
    unsigned char* const t = base + dst * pitch;
    const unsigned j = u - first;
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
  move_feat_rows<SDC_CLONE_FEAT_ROWS>(from, rs, to, rs, rows0, P.feat_rows);
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
