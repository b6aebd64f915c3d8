// sdc_minibatch.hip -- sdc_permutation_kernel, sdc_gather_rows_kernel, sdc_value_norm_sums_kernel, sdc_value_norm_update_kernel and
// sdc_value_loss_normed_kernel: a keyed permutation of row indices, the rows of several arrays gathered by index into dense
// mini-batch arrays, ValueNorm's running update with the critic's scale and shift behind it, and the value loss against the
// handle's own ValueNorm, for sdc_permutation, sdc_gather_rows, sdc_value_norm_update and sdc_value_loss_normed (sdc_capi.hip; the
// plans, the lane mappings and the address bounds: sdc_minibatch_dev.hpp; the arithmetic, shared with a host compiler:
// sdc_minibatch.hpp; the contract: include/sustaindc_hip.h TRAIN ON THE DEVICE).
//
// fp32 with nothing fused (the library is built with -ffp-contract=off; the pragma below says it for this file whatever the flags),
// division and square root correctly rounded (hipcc's default for fp32); the sums are fp64 in a fixed order.
#include <hip/hip_runtime.h>

#include "sdc_minibatch_dev.hpp"

#pragma clang fp contract(off)

#include "sdc_value_loss_dev.hpp"

extern "C" __global__ void __launch_bounds__(SDC_PERM_BLOCK) sdc_permutation_kernel(SdcPermutation P) {
  const unsigned i = blockIdx.x * SDC_PERM_BLOCK + threadIdx.x;      // (n <= 2^31 - 1: the grid's last lane is below 2^31 + 256)
  if (i < P.key.n) P.perm[i] = (int32_t)sdc_perm_index(i, P.key);
}

extern "C" __global__ void __launch_bounds__(SDC_GATHER_BLOCK) sdc_gather_rows_kernel(SdcGatherRows P) {
  __shared__ SdcGatherSeg seg[SDC_GATHER_MAX_SEGMENTS];
  const int t = (int)threadIdx.x;
  if (t < P.n_segs) seg[t] = P.seg[t];
  __syncthreads();
  constexpr int WAVES = SDC_GATHER_BLOCK / 64;
  const int lane = t & 63;
  const long long stride = (long long)gridDim.x * WAVES;
  for (long long k = (long long)blockIdx.x * WAVES + (t >> 6); k < P.n_rows; k += stride) {
    // (one address for the wavefront: one request; the value is the same in every lane)
    const int r = __builtin_amdgcn_readfirstlane(P.idx[k]);
    const bool ok = (unsigned)r < P.n_src_rows;
    if (!ok && lane == 0 && P.bad) P.bad[0] = 1;
    for (int d = lane; d < P.row_dwords; d += 64) {
      int s = 0;
      for (int q = 1; q < P.n_segs; q++) s = d >= seg[q].first ? q : s;
      const SdcGatherSeg g = seg[s];
      const int j = d - g.first;
      uint32_t v = 0u;
      if (ok) v = g.src[(long long)r * g.src_stride + j];
      g.dst[k * g.dst_stride + j] = v;
    }
  }
}

namespace {

// both stages' tree over the workgroup's pairs: lane 0's comes back in (s1, s2)
__device__ __forceinline__ void halve2(double (&part)[2][SDC_VN_BLOCK], double& s1, double& s2, const int l) {
  part[0][l] = s1;
  part[1][l] = s2;
  __syncthreads();
  for (int half = SDC_VN_BLOCK / 2; half >= 1; half >>= 1) {
    if (l < half) {
      part[0][l] = part[0][l] + part[0][l + half];
      part[1][l] = part[1][l] + part[1][l + half];
    }
    __syncthreads();
  }
  s1 = part[0][0];
  s2 = part[1][0];
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_VN_BLOCK) sdc_value_norm_sums_kernel(SdcValueNormSums P) {
  __shared__ double part[2][SDC_VN_BLOCK];
  const int l = (int)threadIdx.x;
  double s1, s2;
  sdc_value_norm_lane_sums(P.x, P.n, (int)gridDim.x, (int)blockIdx.x, l, s1, s2);
  halve2(part, s1, s2, l);
  if (l == 0) {
    P.part[2 * (size_t)blockIdx.x] = s1;
    P.part[2 * (size_t)blockIdx.x + 1] = s2;
  }
}

extern "C" __global__ void __launch_bounds__(SDC_VN_BLOCK) sdc_value_norm_update_kernel(SdcValueNormUpdate P) {
  __shared__ double part[2][SDC_VN_BLOCK];
  const int l = (int)threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int b = l; b < P.n_part; b += SDC_VN_BLOCK) {
    s1 = s1 + P.part[2 * (size_t)b];
    s2 = s2 + P.part[2 * (size_t)b + 1];
  }
  halve2(part, s1, s2, l);
  if (l == 0) {
    SdcValueNormDev s = *P.block;
    sdc_value_norm_update(s, s1, s2, P.n, P.beta);
    *P.block = s;
    P.critic->scale = s.scale;
    P.critic->shift = s.shift;
  }
}

extern "C" __global__ void __launch_bounds__(SDC_PPO_BLOCK) sdc_value_loss_normed_kernel(SdcValueLoss P, const SdcValueNormDev* block) {
  __shared__ double part[7][SDC_PPO_BLOCK];
  P.scale = (double)block->scale;
  P.shift = (double)block->shift;
  // (sdc_value_loss_kernel's switches: the launch's, the same in every lane)
  const bool huber = (P.flags & SDC_VALUE_LOSS_HUBER) != 0;
  if (P.part) {
    if (huber) value_loss_pass<true, true>(P, part);
    else value_loss_pass<false, true>(P, part);
  } else {
    if (huber) value_loss_pass<true, false>(P, part);
    else value_loss_pass<false, false>(P, part);
  }
}

hipError_t sdc_permutation_launch(const SdcPermutation& P, hipStream_t st) {
  const unsigned blocks = (P.key.n + (SDC_PERM_BLOCK - 1u)) / SDC_PERM_BLOCK;
  hipLaunchKernelGGL(sdc_permutation_kernel, dim3(blocks), dim3(SDC_PERM_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_gather_rows_launch(const SdcGatherRows& P, hipStream_t st) {
  constexpr int WAVES = SDC_GATHER_BLOCK / 64;
  const long long want = (P.n_rows + WAVES - 1) / WAVES;
  const unsigned blocks = (unsigned)(want < SDC_GATHER_MAX_BLOCKS ? want : SDC_GATHER_MAX_BLOCKS);
  hipLaunchKernelGGL(sdc_gather_rows_kernel, dim3(blocks), dim3(SDC_GATHER_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_value_norm_update_launch(const SdcValueNormSums& S, const SdcValueNormUpdate& U, hipStream_t st) {
  hipLaunchKernelGGL(sdc_value_norm_sums_kernel, dim3(U.n_part), dim3(SDC_VN_BLOCK), 0, st, S);
  hipLaunchKernelGGL(sdc_value_norm_update_kernel, dim3(1), dim3(SDC_VN_BLOCK), 0, st, U);
  return hipGetLastError();
}

hipError_t sdc_value_loss_normed_launch(const SdcValueLoss& P, const SdcValueNormDev* block, hipStream_t st) {
  hipLaunchKernelGGL(sdc_value_loss_normed_kernel, dim3(sdc_ppo_blocks(P.n)), dim3(SDC_PPO_BLOCK), 0, st, P, block);
  return hipGetLastError();
}
