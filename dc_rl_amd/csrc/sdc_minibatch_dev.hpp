// sdc_minibatch_dev.hpp -- the launch plans of sdc_minibatch.hip: sdc_permutation_kernel (sdc_permutation), sdc_gather_rows_kernel
// (sdc_gather_rows), sdc_value_norm_sums_kernel and sdc_value_norm_update_kernel (sdc_value_norm_update) and
// sdc_value_loss_normed_kernel (sdc_value_loss_normed).  The arithmetic: sdc_minibatch.hpp and sdc_value_loss_dev.hpp; the contract:
// include/sustaindc_hip.h TRAIN ON THE DEVICE.
//
// sdc_permutation_kernel: ONE LANE PER OUTPUT, ceil(n / 256) workgroups of 256 lanes, lane i < n stores perm[i] = sdc_perm_index(i):
//   ~240 integer operations per Feistel pass, fewer than four passes on average, one coalesced dword store.
//   ADDRESS BOUNDS: i < n = the length of perm.
// sdc_gather_rows_kernel: ONE WAVEFRONT PER DESTINATION ROW at a time, four wavefronts per workgroup, min(ceil(n_rows / 4),
//   SDC_GATHER_MAX_BLOCKS) workgroups in grid stride over the rows.  The segments' dwords of one row are numbered 0 .. D-1 behind each
//   other (D = the sum of n_dwords); lane l takes d = l, l + 64, ... < D: consecutive lanes take consecutive dwords of one source row
//   and one destination row, so a row's segment of w dwords touches ceil(w * 4 / 128) + 1 lines at most on either side.  idx[k] is
//   read once per row at an address the wavefront shares (one request); the segment table (at most 16 entries) is staged in LDS once
//   per workgroup and a lane finds the segment of its dword by comparing against the segments' first dwords.  The gather is bound by
//   the lines it touches: a random source row of 26 or 29 dwords costs two 128-byte lines for 104 or 116 bytes used.
//   ADDRESS BOUNDS: k < n_rows for idx and `dst + k * dst_stride + j`, j < n_dwords <= dst_stride (refused otherwise);
//   r = idx[k] enters an address only behind (unsigned)r < n_src_rows: `src + r * src_stride + j`; else the row's dwords are stored as
//   zero and lane 0 stores 1 into `bad` (a plain vector store).  The caller's arrays hold n_src_rows / n_rows rows of their stride.
// sdc_value_norm_sums_kernel / sdc_value_norm_update_kernel: sdc_ppo_terms' two stages word for word over two sums -- B =
//   sdc_value_norm_blocks(n) workgroups of 256 lanes, lane l of workgroup b folds i = b * 256 + l + k * 256 * B (sdc_value_norm_lane_sums),
//   the tree from 128 down through LDS, lane 0's pair is partial b of the handle's [SDC_VN_MAX_BLOCKS][2]; then ONE workgroup: lane l
//   folds partials l, l + 256, ... < B, the same tree, and lane 0 alone runs sdc_value_norm_update on the handle's block and stores
//   scale and shift into the critic's packed copy as sdc_critic_norm_kernel does.  No atomics.
//   ADDRESS BOUNDS: i < n = the length of returns; b < B <= SDC_VN_MAX_BLOCKS.
// sdc_value_loss_normed_kernel: sdc_value_loss_kernel's launch and body (sdc_value_loss_dev.hpp); scale and shift are two loads from
//   the handle's block in front of it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sdc_critic_grad.hpp"
#include "sdc_critic_pack.hpp"
#include "sdc_minibatch.hpp"

#define SDC_PERM_BLOCK 256
#define SDC_GATHER_BLOCK 256
#define SDC_GATHER_MAX_BLOCKS 4096

static_assert(SDC_VN_BLOCK == SDC_PPO_BLOCK && SDC_VN_MAX_BLOCKS == SDC_PPO_MAX_BLOCKS, "ValueNorm's sums run in sdc_ppo_terms' order");

struct SdcPermutation {
  SdcPermKey key;
  int32_t* perm;                 // [n]
};

struct SdcGatherSeg {
  const uint32_t* src;
  uint32_t* dst;
  long long src_stride, dst_stride;      // dwords
  int first;                     // the segment's first dword in a row's numbering
  int n_dwords;
};
struct SdcGatherRows {
  const int32_t* idx;            // [n_rows]
  long long n_rows;
  unsigned n_src_rows;
  int n_segs;
  int row_dwords;                // D
  int32_t* bad;                  // [1] or nullptr
  SdcGatherSeg seg[SDC_GATHER_MAX_SEGMENTS];
};

struct SdcValueNormSums {
  const float* x;                // [n]
  long long n;
  double* part;                  // [B][2]
};
struct SdcValueNormUpdate {
  int n_part;                    // B
  long long n;
  double beta;
  const double* part;
  SdcValueNormDev* block;
  SdcCriticDev* critic;
};

hipError_t sdc_permutation_launch(const SdcPermutation& P, hipStream_t st);
hipError_t sdc_gather_rows_launch(const SdcGatherRows& P, hipStream_t st);
hipError_t sdc_value_norm_update_launch(const SdcValueNormSums& S, const SdcValueNormUpdate& U, hipStream_t st);
hipError_t sdc_value_loss_normed_launch(const SdcValueLoss& P, const SdcValueNormDev* block, hipStream_t st);
