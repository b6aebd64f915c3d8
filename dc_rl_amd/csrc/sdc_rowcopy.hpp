// sdc_rowcopy.hpp -- what the row-copy kernels share: sdc_clone.hip (env -> env), sdc_snapshot.hip (env <-> snapshot row) and
// sdc_mark.hip (env <-> mark row).  The segment table of the env-major arrays and its scan, the 16-byte vector the copies move, the
// clearing of a copied header's re-centring stamps, and the mover of the step-major feature rows.
#pragma once

#include "sdc_device.hpp"

// one env-major array: env e's row starts at base + e * pitch; its units are numbered from `first` on within the segment's class
// (`wide`: 16-byte units, base and pitch 16-byte aligned; `narrow`: dwords)
struct SdcSeg {
  unsigned char* base;
  unsigned pitch;
  unsigned first;
};

// (a clang vector, not HIP's uint4: an array of HIP's vector struct is not promoted to registers -- a feature-row mover's eight loads
// went through scratch memory)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the segment unit u of a class lies in: the last one whose first unit is <= u (the unit is the segment's unit u - first).  The scan is
// unrolled over the table's capacity, so every segment is read at a constant index (a runtime index into the by-value plan would put
// the plan in scratch memory)
template <int CAP>
__device__ __forceinline__ void seg_find(const SdcSeg (&T)[CAP], const int n_segs, const unsigned u, unsigned char*& base, unsigned& pitch,
                                         unsigned& first, int& seg) {
  unsigned char* b = T[0].base;
  unsigned p = T[0].pitch, f = 0;
  seg = 0;
#pragma unroll
  for (int i = 1; i < CAP; i++)
    if (i < n_segs && T[i].first <= u) {
      b = T[i].base;
      p = T[i].pitch;
      f = T[i].first;
      seg = i;
    }
  base = b;
  pitch = p;
  first = f;
}

// 16-byte unit `unit` of a table in which a per-env header starts at unit `header_first`, on its way into a copy: dwords H_PEND .. H_PEND + 3 become zeros, i.e. no deferred
// re-centring in flight.  A request carries its env's index and the launch counter of the engine and the moment that filed it: a clone's
// dst must not take over src's, a snapshot or mark row describes no launch at all, and a restored or rewound env's former state no
// longer exists.  (The windows themselves are copied and valid as they are.)
__device__ __forceinline__ u32x4 clear_pend(u32x4 v, const unsigned unit, const unsigned header_first = 0) {
  static_assert(H_PEND % 4 == 2, "H_PEND .. H_PEND + 3 are the last two dwords of one 16-byte unit and the first two of the next");
  if (unit == header_first + H_PEND / 4) { v.z = 0u; v.w = 0u; }
  if (unit == header_first + H_PEND / 4 + 1) { v.x = 0u; v.y = 0u; }
  return v;
}

// one lane's 16-byte piece of ROWS consecutive feature rows from rows0 on: from[row * from_stride] -> to[row * to_stride] (strides in
// 16-byte units: N * 8 in SdcDev::feat, 8 in a snapshot row).  Rows past the end are clamped to the last row, which the lane then
// copies more than once: no branches between the loads and the stores, so the loads stay in flight together
template <int ROWS>
__device__ __forceinline__ void move_feat_rows(const u32x4* from, const size_t from_stride, u32x4* to, const size_t to_stride,
                                               const int rows0, const int n_rows) {
  u32x4 v[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; i++) v[i] = from[(size_t)min(rows0 + i, n_rows - 1) * from_stride];
#pragma unroll
  for (int i = 0; i < ROWS; i++) to[(size_t)min(rows0 + i, n_rows - 1) * to_stride] = v[i];
}
