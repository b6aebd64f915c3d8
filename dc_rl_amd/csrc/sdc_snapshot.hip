// sdc_snapshot.hip -- sdc_snapshot_save_kernel: env envs[k] -> snapshot row k; sdc_snapshot_restore_kernel: snapshot row rows[k] ->
// env envs[k] (sdc_snapshot_envs / sdc_restore_envs, sdc_capi.hip; the plan and the row layout: sdc_snapshot.hpp).
//
// Bandwidth kernels built from the same parts as sdc_clone.hip (sdc_rowcopy.hpp): a row is 145 920 bytes at 672-step episodes (sdc_capi.hip snap_plan: ring 40 960,
// feature rows 86 144, weather windows 2 x 5 520, queue table 5 632, record + header + rank windows 1 536, obs rows 428, padding to
// 256), each byte read once and written once.  Reads and writes never meet: the save
// reads the engine and writes the caller's rows, the restore reads the rows and writes the engine, and the host refuses a dst that
// appears twice, so no two lanes write the same byte.  The save is READ-ONLY on the engine: the header's re-centring stamps (H_PEND)
// go into the row as zeros and stay as they are in the live env, so taking a snapshot does not change the run it is taken from.
// The mirrors (qcum_t, hist_t) and the per-env config scalars (prm_env) are derived data: the restore rebuilds them from the row.
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_snapshot.hpp"

namespace {

// record dwords R_CFG / R_LOC of a restored env: the assignment the host checked against this engine's configs and trace sets
__device__ __forceinline__ u32x4 set_assignment(u32x4 v, const unsigned unit, const int cfg, const int loc) {
  static_assert(R_CFG % 4 == 0 && R_LOC == R_CFG + 1, "R_CFG, R_LOC: the first two dwords of one 16-byte unit");
  if (unit == R_CFG / 4) { v.x = (unsigned)cfg; v.y = (unsigned)loc; }
  return v;
}

template <bool SAVE>
__device__ __forceinline__ void range_a(const SdcSnapPlan& P, const int b, const int tid) {
  const int k = b / P.bpe, part = b - k * P.bpe;
  const int4 ix = P.idx[k];
  const size_t env = (size_t)ix.x;
  unsigned char* row = P.rows + (size_t)ix.y * P.row_bytes;
  const unsigned stride = (unsigned)P.bpe * SDC_SNAP_BLOCK;
  // 16-byte units: SDC_SNAP_UNROLL loads in flight per lane before the stores
#pragma unroll 1
  for (unsigned u0 = (unsigned)part * SDC_SNAP_BLOCK + tid; u0 < P.wide_units; u0 += SDC_SNAP_UNROLL * stride) {
    u32x4 v[SDC_SNAP_UNROLL];
    u32x4* to[SDC_SNAP_UNROLL];
    unsigned jj[SDC_SNAP_UNROLL];
    int seg[SDC_SNAP_UNROLL];
#pragma unroll
    for (int i = 0; i < SDC_SNAP_UNROLL; i++) {
      const unsigned u = min(u0 + i * stride, P.wide_units - 1);     // (past the end: the last unit again, copied twice)
      unsigned char* base;
      unsigned pitch, first;
      seg_find(P.wide, P.n_wide, u, base, pitch, first, seg[i]);
      jj[i] = u - first;
      unsigned char *const e = base + env * pitch + (size_t)jj[i] * 16, *const s = row + (size_t)u * 16;
      v[i] = *reinterpret_cast<const u32x4*>(SAVE ? e : s);
      to[i] = reinterpret_cast<u32x4*>(SAVE ? s : e);
    }
#pragma unroll
    for (int i = 0; i < SDC_SNAP_UNROLL; i++) {
      u32x4 w = seg[i] == SDC_SNAP_SEG_HDR ? clear_pend(v[i], jj[i]) : v[i];
      if (!SAVE && seg[i] == SDC_SNAP_SEG_REC) w = set_assignment(w, jj[i], ix.z, ix.w);
      *to[i] = w;
    }
  }
  // dword units (rows whose length or alignment is not a multiple of 16 bytes: the observation rows), behind the wide ones in the row;
  // a restored observation row goes to the closed loop's copy as well
  unsigned char* row_n = row + (size_t)P.wide_units * 16;
#pragma unroll 1
  for (unsigned u = (unsigned)part * SDC_SNAP_BLOCK + tid; u < P.narrow_units; u += stride) {
    unsigned char* base;
    unsigned pitch, first;
    int seg;
    seg_find(P.narrow, P.n_narrow, u, base, pitch, first, seg);
    const unsigned j = u - first;
    unsigned char *const e = base + env * pitch + (size_t)j * 4, *const s = row_n + (size_t)u * 4;
    const unsigned w = *reinterpret_cast<const unsigned*>(SAVE ? e : s);
    *reinterpret_cast<unsigned*>(SAVE ? s : e) = w;
    if (!SAVE && seg == SDC_SNAP_SEG_OBS && P.obs_latch) reinterpret_cast<unsigned*>(P.obs_latch + env * SDC_OBS_OUT)[j] = w;
  }
}

template <bool SAVE>
__device__ __forceinline__ void range_b(const SdcSnapPlan& P, const int b, const int tid) {
  const int grp = b % P.feat_groups, rows0 = (b / P.feat_groups) * SDC_SNAP_FEAT_ROWS;
  const int k = grp * (SDC_SNAP_BLOCK / 8) + tid / 8, q = tid & 7;     // env, 16-byte quarter-line of its 128-byte row
  if (k >= P.n) return;
  const int4 ix = P.idx[k];
  constexpr int Q = SDC_FEAT_ROW / 4;      // 16-byte units per feature row
  static_assert(Q == 8, "eight lanes per 128-byte feature row");
  const size_t rs = (size_t)P.n_envs * Q;  // units per step
  u32x4* fe = reinterpret_cast<u32x4*>(P.feat) + (size_t)ix.x * Q + q;
  u32x4* sn = reinterpret_cast<u32x4*>(P.rows + (size_t)ix.y * P.row_bytes + P.feat_off) + q;
  if (SAVE)
    move_feat_rows<SDC_SNAP_FEAT_ROWS>(fe, rs, sn, Q, rows0, P.feat_rows);
  else
    move_feat_rows<SDC_SNAP_FEAT_ROWS>(sn, Q, fe, rs, rows0, P.feat_rows);
}

constexpr int TILE_DW = SDC_SNAP_TILE_BYTES / 4;     // dwords of one env's row per tile
constexpr int PIECES = SDC_SNAP_TILE_BYTES / 16;     // 16-byte loads per env and tile

// one tile of the mirror rebuild: 64 dst envs x 128 bytes of their rows (16 queue-table slots {cum, cumT} or 32 ring keys).  Eight
// lanes read an env's 128 bytes (whole lines), the tile goes through LDS (rows padded by a dword: the column reads below hit 32
// different banks), and each wavefront store writes one mirror row's dwords of 64 consecutive envs (the envs are sorted by dst)
__device__ __forceinline__ void range_c(const SdcSnapPlan& P, const int b, const int tid, unsigned (*tile)[TILE_DW + 1]) {
  static_assert(SDC_SNAP_TILE_ENVS * PIECES == 2 * SDC_SNAP_BLOCK, "two 16-byte loads per lane fill a tile");
  const int tiles = P.q_tiles + P.h_tiles;
  const int grp = b / tiles, t = b - grp * tiles;
  const bool qt = t < P.q_tiles;
  const int k0 = grp * SDC_SNAP_TILE_ENVS;
  const unsigned off = qt ? P.qtab_off + (unsigned)t * SDC_SNAP_TILE_BYTES : P.hist_off + (unsigned)(t - P.q_tiles) * SDC_SNAP_TILE_BYTES;
  u32x4 v[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int c = tid + i * SDC_SNAP_BLOCK, el = c / PIECES, p = c % PIECES;
    const int k = min(k0 + el, P.n - 1);     // (envs past the end: the last one's row again, never written out)
    v[i] = reinterpret_cast<const u32x4*>(P.rows + (size_t)P.idx[k].y * P.row_bytes + off)[p];
  }
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int c = tid + i * SDC_SNAP_BLOCK, el = c / PIECES, p = c % PIECES;
    tile[el][4 * p] = v[i].x;
    tile[el][4 * p + 1] = v[i].y;
    tile[el][4 * p + 2] = v[i].z;
    tile[el][4 * p + 3] = v[i].w;
  }
  __syncthreads();
  const int el = tid & (SDC_SNAP_TILE_ENVS - 1), k = k0 + el;
  if (k >= P.n) return;
  const size_t N = (size_t)P.n_envs, dst = (size_t)P.idx[k].x;
  constexpr int ROWS_PER_PASS = SDC_SNAP_BLOCK / SDC_SNAP_TILE_ENVS;
  if (qt) {     // queue table: the `cum` column, dword 2s of slot s
    const size_t r0 = (size_t)t * (TILE_DW / 2);
#pragma unroll
    for (int s = tid / SDC_SNAP_TILE_ENVS; s < TILE_DW / 2; s += ROWS_PER_PASS) P.qcum_t[(r0 + s) * N + dst] = tile[el][2 * s];
  } else {      // ring: every key up to hist_cap
    const int r0 = (t - P.q_tiles) * TILE_DW;
#pragma unroll
    for (int s = tid / SDC_SNAP_TILE_ENVS; s < TILE_DW; s += ROWS_PER_PASS)
      if (r0 + s < P.hist_cap) P.hist_t[(size_t)(r0 + s) * N + dst] = tile[el][s];
  }
}

// (restore, several configs) every restored env's copy of its config's scalars (SdcDev::prm_env): 256 bytes, sixteen lanes per env
__device__ __forceinline__ void range_d(const SdcSnapPlan& P, const int b, const int tid) {
  const int k = b * (SDC_SNAP_BLOCK / 16) + tid / 16, q = tid & 15;
  if (k >= P.n) return;
  const int4 ix = P.idx[k];
  reinterpret_cast<u32x4*>(P.prm_env + (size_t)ix.x * 32)[q] = reinterpret_cast<const u32x4*>(P.prm_cfg + (size_t)ix.z * 32)[q];
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_SNAP_BLOCK) sdc_snapshot_save_kernel(SdcSnapPlan P) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (b < P.blocks_a)
    range_a<true>(P, b, tid);
  else
    range_b<true>(P, b - P.blocks_a, tid);
}

extern "C" __global__ void __launch_bounds__(SDC_SNAP_BLOCK) sdc_snapshot_restore_kernel(SdcSnapPlan P) {
  __shared__ unsigned tile[SDC_SNAP_TILE_ENVS][TILE_DW + 1];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (b < P.blocks_a)
    range_a<false>(P, b, tid);
  else if (b < P.blocks_a + P.blocks_b)
    range_b<false>(P, b - P.blocks_a, tid);
  else if (b < P.blocks_a + P.blocks_b + P.blocks_c)
    range_c(P, b - P.blocks_a - P.blocks_b, tid, tile);
  else
    range_d(P, b - P.blocks_a - P.blocks_b - P.blocks_c, tid);
}

// the grid of a plan: range A, then B, then (restore) C and D
hipError_t sdc_snapshot_launch(const SdcSnapPlan& P, const bool save, hipStream_t st) {
  if (save)
    hipLaunchKernelGGL(sdc_snapshot_save_kernel, dim3(P.blocks_a + P.blocks_b), dim3(SDC_SNAP_BLOCK), 0, st, P);
  else
    hipLaunchKernelGGL(sdc_snapshot_restore_kernel, dim3(P.blocks_a + P.blocks_b + P.blocks_c + P.blocks_d), dim3(SDC_SNAP_BLOCK), 0, st,
                       P);
  return hipGetLastError();
}
