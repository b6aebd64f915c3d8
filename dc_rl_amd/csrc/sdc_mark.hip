// sdc_mark.hip -- sdc_mark_save_kernel: what the next max_steps env-steps can change in env envs[k] -> mark row k; sdc_mark_rewind_kernel:
// mark row k -> env envs[k], the same slot it was taken from (sdc_mark_envs / sdc_rewind_envs, sdc_capi.hip; the row layout and the block
// ranges: sdc_mark.hpp).
//
// Bandwidth kernels like those of sdc_snapshot.hip, for rows of 2-5 KB instead of 146 KB: every byte is read once and written once,
// every load of a lane is issued before its first store, and reads and writes never meet -- the save reads the engine and writes the
// caller's rows, the rewind reads the rows and writes the engine, and the host refuses an env that appears twice.  (Where hist_cap is
// smaller than max_steps the slot sequence passes a ring slot more than once: the save then reads it more than once, and the rewind's
// lanes write the same saved value to it.)  The save is READ-ONLY on the engine: the header's re-centring stamps (H_PEND) go into the row
// as zeros and stay as they are in the live env.  Every index a kernel derives from a record -- the live one or the row's -- is brought
// into its array's range before it is used (ring_slot: modulo hist_cap; queue entries: below the table's stride), so a row that was
// overwritten by its owner cannot send a store outside the engine's arrays.
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_mark.hpp"
#include "sdc_rowcopy.hpp"

namespace {

constexpr int REC_UNITS = SDC_REC_DWORDS / 4, HDR_UNITS = SDC_HDR_DWORDS / 4, WIN_UNITS = SDC_WIN;
static_assert(REC_UNITS + HDR_UNITS + WIN_UNITS == SDC_MARK_WIDE_UNITS && SDC_OBS_OUT + SDC_SHARE_OBS_DIM == SDC_MARK_OBS_DWORDS &&
              16 * SDC_MARK_WIDE_UNITS + 4 * SDC_MARK_OBS_DWORDS == SDC_MARK_FIXED_BYTES, "the row's fixed part");
static_assert(SDC_MARK_WIDE_UNITS <= 96 && SDC_MARK_WIDE_UNITS > 64 && SDC_MARK_OBS_DWORDS <= 128 && SDC_MARK_OBS_DWORDS > 64,
              "a wavefront moves the fixed part in two passes of each kind");
static_assert(R_TREL == 1 && R_HIST_LEN == 13 && R_HIST_POS == 14, "lane 0 holds t_rel in .y, lane 3 hist_len / hist_pos in .y / .z");

// the ring slot the j-th append after a record with (hist_len, hist_pos) goes to: what j + 1 calls of hist_append_slot (sdc_physics.hpp)
// return last -- hist_len + j while the ring is young, then hist_pos, hist_pos + 1, ... modulo hist_cap.  Always below hist_cap
__device__ __forceinline__ unsigned ring_slot(const int hist_len, const int hist_pos, const int hist_cap, const int j) {
  const int hl = min(max(hist_len, 0), hist_cap), young = hist_cap - hl;
  return j < young ? (unsigned)(hl + j) : ((unsigned)hist_pos + (unsigned)(j - young)) % (unsigned)hist_cap;
}

// unit u of an env's record | header | rank windows, in the engine
__device__ __forceinline__ u32x4* wide_ptr(const SdcMarkPlan& P, const size_t env, const unsigned u) {
  unsigned* p = u < REC_UNITS ? P.rec + env * SDC_REC_DWORDS + 4 * u
                : u < REC_UNITS + HDR_UNITS ? P.hdr + env * SDC_HDR_DWORDS + 4 * (u - REC_UNITS)
                                            : P.qwin + env * (4 * SDC_WIN) + 4 * (u - REC_UNITS - HDR_UNITS);
  return reinterpret_cast<u32x4*>(p);
}

__device__ __forceinline__ void env_row(const SdcMarkPlan& P, const int k, size_t& env, unsigned char*& row) {
  size_t r = (size_t)k;
  env = r;
  if (P.idx) {
    const int4 ix = P.idx[k];
    env = (size_t)ix.x;
    r = (size_t)ix.y;
  }
  row = P.rows + r * P.row_bytes;
}

template <bool SAVE>
__device__ __forceinline__ void range_a(const SdcMarkPlan& P, const int b, const int tid) {
  const int k = b * SDC_MARK_ENVS_PER_BLOCK + (tid >> 6), lane = tid & 63;
  if (k >= P.n) return;     // (the whole wavefront)
  size_t env;
  unsigned char* row;
  env_row(P, k, env, row);
  // ---- the fixed part: every lane's loads first
  const unsigned u0 = (unsigned)lane, u1 = 64u + (unsigned)(lane & 31);     // (lanes 32 .. 63: unit u1 again, never stored)
  const unsigned d0 = (unsigned)lane, d1 = min(64u + (unsigned)lane, (unsigned)SDC_MARK_OBS_DWORDS - 1u);
  u32x4* const rw = reinterpret_cast<u32x4*>(row);
  unsigned* const rn = reinterpret_cast<unsigned*>(row + 16 * SDC_MARK_WIDE_UNITS);
  u32x4* const e0 = wide_ptr(P, env, u0);
  u32x4* const e1 = wide_ptr(P, env, u1);
  const auto narrow_ptr = [&P, env](const unsigned d) {
    return reinterpret_cast<unsigned*>(d < SDC_OBS_OUT ? P.obs + env * SDC_OBS_OUT + d : P.share_obs + env * SDC_SHARE_OBS_DIM + (d - SDC_OBS_OUT));
  };
  unsigned* const f0 = narrow_ptr(d0);
  unsigned* const f1 = narrow_ptr(d1);
  u32x4 w0 = SAVE ? *e0 : rw[u0];
  const u32x4 w1 = SAVE ? *e1 : rw[u1];
  const unsigned n0 = SAVE ? *f0 : rn[d0], n1 = SAVE ? *f1 : rn[d1];
  // the record's episode step and ring position: lanes 0 and 3 hold them (the live record on a save, the saved one on a rewind)
  const int t_rel = __builtin_amdgcn_readlane((int)w0.y, 0);
  const int hist_len = __builtin_amdgcn_readlane((int)w0.y, 3), hist_pos = __builtin_amdgcn_readlane((int)w0.z, 3);
  w0 = clear_pend(w0, u0, REC_UNITS);     // (the header follows the record)

  // ---- the variable part: K ring slots, then K queue-table entries of two dwords; SDC_MARK_VAR_UNROLL loads in flight per lane.  The
  // fixed part's stores follow the first pass's loads
  const unsigned K = (unsigned)P.max_steps, nvar = 3u * K, qstride = (unsigned)P.qstride;
  unsigned* const rv = reinterpret_cast<unsigned*>(row + SDC_MARK_FIXED_BYTES);
  unsigned* const ring = P.hist + env * SDC_HIST_STRIDE;
  unsigned* const qt = P.qtab + env * (size_t)qstride * 2;
  bool fixed_done = false;
  unsigned v0 = (unsigned)lane;
#pragma unroll 1
  do {
    unsigned x[SDC_MARK_VAR_UNROLL];
    unsigned* eng[SDC_MARK_VAR_UNROLL];
    unsigned* sav[SDC_MARK_VAR_UNROLL];
    bool ok[SDC_MARK_VAR_UNROLL];
#pragma unroll
    for (int i = 0; i < SDC_MARK_VAR_UNROLL; i++) {
      const unsigned v = min(v0 + 64u * i, nvar - 1u);     // (past the end: the last dword again, copied twice)
      const unsigned q = v - K, tq = (unsigned)t_rel + (q >> 1);
      const bool is_ring = v < K;
      ok[i] = is_ring || tq < qstride;     // (queue entries past the table: a mark near the episode's end has fewer than K steps left)
      eng[i] = is_ring ? ring + ring_slot(hist_len, hist_pos, P.hist_cap, (int)v) : qt + 2u * min(tq, qstride - 1u) + (q & 1u);
      sav[i] = rv + v;
      x[i] = *(SAVE ? eng[i] : sav[i]);
    }
    if (!fixed_done) {
      fixed_done = true;
      if (SAVE) {
        rw[u0] = w0;
        if (lane < 32) rw[u1] = w1;
        rn[d0] = n0;
        if (lane + 64 < SDC_MARK_OBS_DWORDS) rn[d1] = n1;
      } else {
        *e0 = w0;
        if (lane < 32) *e1 = w1;
        *f0 = n0;
        if (lane + 64 < SDC_MARK_OBS_DWORDS) *f1 = n1;
        // a rewound observation row goes to the closed loop's copy as well
        if (P.obs_latch) {
          unsigned* const latch = reinterpret_cast<unsigned*>(P.obs_latch + env * SDC_OBS_OUT);
          latch[d0] = n0;
          if (d1 < SDC_OBS_OUT && lane + 64 < SDC_MARK_OBS_DWORDS) latch[d1] = n1;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < SDC_MARK_VAR_UNROLL; i++) {
      if (SAVE)
        *sav[i] = ok[i] ? x[i] : 0u;
      else if (ok[i])
        *eng[i] = x[i];
    }
    v0 += SDC_MARK_VAR_UNROLL * 64u;
  } while (v0 < nvar);
}

// the mirrors' rows of the rewound slots: a lane per env, SDC_MARK_MIRROR_J steps per workgroup; everything comes from the row
__device__ __forceinline__ void range_m(const SdcMarkPlan& P, const int b, const int tid) {
  const int grp = b / P.m_chunks, chunk = b - grp * P.m_chunks;
  const int k = grp * SDC_MARK_BLOCK + tid;
  if (k >= P.n) return;
  size_t env;
  unsigned char* row;
  env_row(P, k, env, row);
  const unsigned* const r = reinterpret_cast<const unsigned*>(row);
  const unsigned* const rv = reinterpret_cast<const unsigned*>(row + SDC_MARK_FIXED_BYTES);
  const int K = P.max_steps, j0 = chunk * SDC_MARK_MIRROR_J;
  const int t_rel = (int)r[R_TREL], hist_len = (int)r[R_HIST_LEN], hist_pos = (int)r[R_HIST_POS];
  unsigned cum[SDC_MARK_MIRROR_J], key[SDC_MARK_MIRROR_J];
#pragma unroll
  for (int i = 0; i < SDC_MARK_MIRROR_J; i++) {
    const int j = min(j0 + i, K - 1);     // (steps past K: the last one's again, never written out)
    cum[i] = rv[K + 2 * j];
    key[i] = rv[j];
  }
  const size_t N = (size_t)P.n_envs;
#pragma unroll
  for (int i = 0; i < SDC_MARK_MIRROR_J; i++) {
    const int j = j0 + i;
    if (j >= K) continue;
    const unsigned tq = (unsigned)t_rel + (unsigned)j;
    if (tq < (unsigned)P.qstride) P.qcum_t[(size_t)tq * N + env] = cum[i];
    if (P.hist_t) P.hist_t[(size_t)ring_slot(hist_len, hist_pos, P.hist_cap, j) * N + env] = key[i];
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_MARK_BLOCK) sdc_mark_save_kernel(SdcMarkPlan P) {
  range_a<true>(P, (int)blockIdx.x, (int)threadIdx.x);
}

extern "C" __global__ void __launch_bounds__(SDC_MARK_BLOCK) sdc_mark_rewind_kernel(SdcMarkPlan P) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (b < P.blocks_a)
    range_a<false>(P, b, tid);
  else
    range_m(P, b - P.blocks_a, tid);
}

// the grid of a plan: range A, then (rewind) M
hipError_t sdc_mark_launch(const SdcMarkPlan& P, const bool save, hipStream_t st) {
  if (save)
    hipLaunchKernelGGL(sdc_mark_save_kernel, dim3(P.blocks_a), dim3(SDC_MARK_BLOCK), 0, st, P);
  else
    hipLaunchKernelGGL(sdc_mark_rewind_kernel, dim3(P.blocks_a + P.blocks_m), dim3(SDC_MARK_BLOCK), 0, st, P);
  return hipGetLastError();
}
