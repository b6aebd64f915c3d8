// sdc_clone.hpp -- the copy plan sdc_clone_envs (sdc_capi.hip) hands to sdc_clone_kernel (sdc_clone.hip).
//
// One launch copies env src[k]'s state onto env dst[k] for every pair k, in three block ranges:
//   A  the ENV-MAJOR arrays (a row of `pitch` bytes per env: record, header, ring, rank windows, queue table, weather windows,
//      per-env config scalars, the closed loop's observation copy, the caller's obs / share_obs): `bpp` workgroups per pair,
//      16 bytes per lane where the row allows it (SdcSeg in `wide`, sdc_rowcopy.hpp), a dword per lane where it does not;
//   B  the STEP-MAJOR feature rows (SdcDev::feat, [episode_steps + 1][N][SDC_FEAT_ROW]): a 128-byte row per (step, pair), eight
//      lanes of 16 bytes each, 32 pairs and SDC_CLONE_FEAT_ROWS steps per workgroup;
//   C  the SLOT-MAJOR mirrors (SdcDev::qcum_t and, behind it in the same allocation, SdcDev::hist_t: [rows][N] dwords): a lane
//      per pair, 256 consecutive pairs (sorted by dst: a contiguous dst range writes whole lines) and SDC_CLONE_MIRROR_ROWS rows
//      per workgroup.
#pragma once

#include "sdc_rowcopy.hpp"

#define SDC_CLONE_BLOCK 256
#define SDC_CLONE_MAX_WIDE 8        // segments of 16-byte units (record, header, ring, windows, queue table, weather windows, config scalars)
#define SDC_CLONE_MAX_NARROW 6      // segments of dwords (observation rows; weather windows of an odd length)
#define SDC_CLONE_UNROLL 4          // wide units a lane loads before it stores (range A)
#define SDC_CLONE_FEAT_ROWS 8       // steps per workgroup (range B)
#define SDC_CLONE_MIRROR_ROWS 16    // mirror rows per workgroup (range C)

struct SdcClonePlan {
  const int2* pairs;       // [n] {src, dst}, sorted by dst (device)
  int n;                   // pairs
  int n_envs;
  int n_wide, n_narrow;
  int hdr_wide;            // which wide segment is the per-env header (the copy clears its re-centring stamps, H_PEND)
  unsigned wide_units, narrow_units;   // per pair, over all segments of the class
  SdcSeg wide[SDC_CLONE_MAX_WIDE];
  SdcSeg narrow[SDC_CLONE_MAX_NARROW];
  int bpp;                 // range A: workgroups per pair
  int blocks_a, blocks_b;  // range A's workgroups, range B's: the grid is A, then B, then C
  float* feat;             // range B (nullptr: none)
  int feat_rows;           // episode_steps + 1
  int feat_pair_groups;    // ceil(n / 32)
  unsigned* mirror;        // range C (nullptr: none): [mirror_rows][n_envs]
  int mirror_rows;
  int mirror_pair_groups;  // ceil(n / 256)
};

hipError_t sdc_clone_launch(const SdcClonePlan& P, hipStream_t st);
