// sdc_snapshot.hpp -- the plans sdc_snapshot_envs / sdc_restore_envs (sdc_capi.hip) hand to sdc_snapshot_save_kernel and
// sdc_snapshot_restore_kernel (sdc_snapshot.hip).
//
// A snapshot row is one env's complete state in a layout that depends on the state layout and on episode_steps alone (the ring's
// stride is fixed; the queue table's and the weather windows' lengths and the feature rows follow from episode_steps) -- never on
// the engine's n_envs or mapping.  Rows are row_bytes apart (a multiple of 256) in a caller-owned device buffer [n_rows][row_bytes].
// One launch per direction, in block ranges:
//   A  the ENV-MAJOR arrays (record, header, rank windows, caller obs / share_obs, queue table, weather windows, ring): `bpe`
//      workgroups per env, 16 bytes per lane where the engine's row allows it (SdcSeg in `wide`, sdc_rowcopy.hpp), a dword per lane where it
//      does not (`narrow`);
//   B  the STEP-MAJOR feature rows (SdcDev::feat [episode_steps + 1][N][SDC_FEAT_ROW]) <-> episode_steps + 1 contiguous 128-byte rows
//      of the snapshot row: eight lanes of 16 bytes per row, 32 envs and SDC_SNAP_FEAT_ROWS steps per workgroup;
//   C  (restore only) the SLOT-MAJOR mirrors (SdcDev::qcum_t, SdcDev::hist_t: [rows][N] dwords), rebuilt from the snapshot row's
//      queue table and ring: a tile of 64 envs x 128 bytes of their rows is read whole lines into LDS and written out mirror row by
//      mirror row, 64 consecutive (dst-sorted) envs per wavefront store;
//   D  (restore, several configs) the per-env copy of the config's scalars (SdcDev::prm_env), from a per-config table.
#pragma once

#include "sdc_rowcopy.hpp"

#define SDC_SNAP_BLOCK 256
#define SDC_SNAP_MAX_WIDE 7         // segments of 16-byte units (record, header, rank windows, queue table, weather windows, ring)
#define SDC_SNAP_MAX_NARROW 4       // segments of dwords (observation rows; weather windows of an odd length)
#define SDC_SNAP_UNROLL 4           // wide units a lane loads before it stores (range A)
#define SDC_SNAP_FEAT_ROWS 8        // steps per workgroup (range B)
#define SDC_SNAP_TILE_ENVS 64       // envs per mirror tile (range C): one wavefront store of 64 dwords per mirror row
#define SDC_SNAP_TILE_BYTES 128     // bytes of each env's snapshot row per tile: 16 queue-table slots or 32 ring slots
#define SDC_SNAP_SEG_REC 0          // the first wide segment is the record (restore: cfg_id / loc_id come from the host-checked manifest),
#define SDC_SNAP_SEG_HDR 1          // the second the header (its re-centring stamps H_PEND are written as zeros, both ways)
#define SDC_SNAP_SEG_OBS 0          // the first narrow segment is the caller's obs (restore: written to the closed loop's copy too)

// env e's unit j of a segment lies at base + e * pitch + j * unit (unit: 16 bytes in `wide`, 4 in `narrow`).  In a snapshot row the
// wide units lie in unit order from byte 0 on, the narrow ones from byte 16 * wide_units on (a class's segments in unit order: no row
// offset per segment), the feature rows at feat_off

struct SdcSnapPlan {
  const int4* idx;         // [n] {env, snapshot row, cfg_id, loc_id} (device; restore: sorted by env)
  int n;
  int n_envs;
  unsigned char* rows;     // the caller's buffer [n_rows][row_bytes]
  unsigned row_bytes;
  int n_wide, n_narrow;
  unsigned wide_units, narrow_units;   // per env, over all segments of the class
  SdcSeg wide[SDC_SNAP_MAX_WIDE];
  SdcSeg narrow[SDC_SNAP_MAX_NARROW];
  int bpe;                 // range A: workgroups per env
  int blocks_a, blocks_b, blocks_c, blocks_d;   // the grid is A, then B, then C, then D
  float* feat;             // range B (nullptr: none)
  int feat_rows;           // episode_steps + 1
  unsigned feat_off;       // the feature rows' offset in a snapshot row
  int feat_groups;         // ceil(n / 32)
  // restore only
  float* obs_latch;        // the closed loop's copy of the latest observations (nullptr: none), written with the caller's obs rows
  const double* prm_cfg;   // range D (blocks_d 0: none): [n_cfg][32] every config's scalars (several configs), copied into dst's
  double* prm_env;         // row of SdcDev::prm_env [N][32], 16 envs per workgroup
  unsigned* qcum_t;        // range C (nullptr: none): [qstride][N]
  unsigned* hist_t;        // [hist_cap][N] (nullptr: no ring mirror; h_tiles 0)
  int qstride, hist_cap;
  unsigned qtab_off, hist_off;   // the queue table's and the ring's offsets in a snapshot row
  int q_tiles, h_tiles;    // tiles per group of 64 envs: qstride / 16, ceil(hist_cap / 32)
  int tile_groups;         // ceil(n / 64)
};

hipError_t sdc_snapshot_launch(const SdcSnapPlan& P, bool save, hipStream_t st);
