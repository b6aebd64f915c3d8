// sdc_critic.hip -- the two kernels over sdc_critic::forward (sdc_critic.hpp; the network, the mapping, the numerics: sdc_rowmlp.hpp):
//   sdc_critic_values_kernel     rows [R][29] in, values [R] out                                     (sdc_critic_values)
//   sdc_critic_terminal_kernel   the N share_obs rows of a plan horizon's last step -> score[n] += factor * (done[n] ? 0 : V[n])
//                                in fp64, no fused multiply-add (the library is built with -ffp-contract=off; the contract:
//                                include/sustaindc_hip.h THE PLAN CRITIC)
//
// The shape of both: workgroups of four wavefronts; the critic (26 KB) is copied from device memory to LDS once per workgroup, then the
// workgroup takes 64 rows per pass, 16 per wavefront, and as many passes as the grid (at most SDC_CRITIC_MAX_BLOCKS workgroups) leaves
// it.  A wavefront's 16 rows are 464 contiguous dwords: they are read densely -- lane l takes dwords l, l + 64, ... -- into the
// wavefront's own LDS tile and picked from there as the B operands (lane (g, e): entries 4 s + g of row e).  Every address a lane
// forms is below its array's end: a dword of a row at or past n_rows is not loaded (the tile gets 0 -- such rows compute on zeros)
// and its value is not stored; the tile's reads stay inside the tile (entries 29..31 of a row are not read: 0).  The number of
// passes is the same in every wavefront of a workgroup (it follows from blockIdx alone), so the barrier of a pass is reached by all.
#include <hip/hip_runtime.h>

#include "sdc_critic.hpp"
#include "sdc_rowmlp.hpp"

namespace {

constexpr int TILE_DW = sdc_rowmlp::TILE_DW<SDC_CRITIC_IN>;           // 464
constexpr int TILE_LOADS = sdc_rowmlp::TILE_LOADS<SDC_CRITIC_IN>;     // 8

using Lds = sdc_rowmlp::Lds<SdcCriticDev, SDC_CRITIC_IN>;
static_assert(sizeof(Lds) <= 40 * 1024, "four workgroups' LDS fit a CU");

// A wavefront's rows row0 .. row0 + 15 of `rows` (n_rows in all), densely: lane l takes dwords l, l + 64, ... of the 464; a dword of
// a row at or past n_rows is not loaded (0).  (Not sdc_rowmlp::fetch: contiguous rows need no division.)
__device__ __forceinline__ void fetch(float (&v)[TILE_LOADS], const float* rows, const long long row0, const long long n_rows, const int lane) {
  const int valid = sdc_rowmlp::rows_that_exist(row0, n_rows) * SDC_CRITIC_IN;      // dwords that exist
  const float* const src = rows + row0 * SDC_CRITIC_IN;
#pragma unroll
  for (int j = 0; j < TILE_LOADS; j++) {
    const int u = lane + 64 * j;
    v[j] = 0.0f;
    if (u < valid) v[j] = src[u];
  }
}

// One pass of a wavefront: the fetched dwords through the wavefront's tile -> the value of row (lane & 15), in every lane of that
// column.  The barrier inside orders the tile's stores (and, in the first pass, the critic's copy) before the reads; the tile is the
// wavefront's own, and LDS operations of one wavefront complete in order, so the next pass's stores need no second barrier.  Behind
// the tile's reads the NEXT pass's rows are fetched (next0; past the grid's last pass: nothing is loaded), under this pass's arithmetic.
__device__ __forceinline__ float pass(Lds& L, float (&v)[TILE_LOADS], const float* rows, const long long next0, const long long n_rows,
                                      const int wave, const int lane) {
#pragma unroll
  for (int j = 0; j < TILE_LOADS; j++) {
    const int u = lane + 64 * j;
    if (u < TILE_DW) L.tile[wave][u] = v[j];
  }
  __syncthreads();
  const int g = lane >> 4, e = lane & 15;
  float x[SDC_CRITIC_S1];
#pragma unroll
  for (int s = 0; s < SDC_CRITIC_S1; s++) {
    const int k = 4 * s + g;
    x[s] = 0.0f;
    if (k < SDC_CRITIC_IN) x[s] = L.tile[wave][e * SDC_CRITIC_IN + k];
  }
  fetch(v, rows, next0, n_rows, lane);
  return sdc_critic::forward(&L.net, x, lane);
}

// the passes of a workgroup over n_rows rows: store(row, value) for every row that exists, by the lane (< 16) that owns it
template <class Store>
__device__ __forceinline__ void passes(Lds& L, const SdcCriticDev* critic, const float* rows, const long long n_rows, Store&& store) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  sdc_rowmlp::to_lds(&L.net, critic);
  const long long n_pass = (n_rows + SDC_CRITIC_BLOCK_ROWS - 1) / SDC_CRITIC_BLOCK_ROWS;
  const long long stride = (long long)gridDim.x * SDC_CRITIC_BLOCK_ROWS;
  long long row0 = (long long)blockIdx.x * SDC_CRITIC_BLOCK_ROWS + wave * SDC_ROWMLP_ROWS;
  float v[TILE_LOADS];
  fetch(v, rows, row0, n_rows, lane);
#pragma unroll 1
  for (long long p = blockIdx.x; p < n_pass; p += gridDim.x, row0 += stride) {
    // (a next pass that does not exist starts at or past n_rows -- the grid's stride is whole workgroups --: fetch loads nothing)
    const float value = pass(L, v, rows, row0 + stride, n_rows, wave, lane);
    const long long row = row0 + lane;
    if (lane < SDC_ROWMLP_ROWS && row < n_rows) store(row, value);
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_CRITIC_BLOCK, SDC_CRITIC_WAVES_PER_SIMD) sdc_critic_values_kernel(SdcCriticValues P) {
  __shared__ Lds L;
  passes(L, P.critic, P.rows, P.n_rows, [&](const long long row, const float v) { P.values[row] = v; });
}

extern "C" __global__ void __launch_bounds__(SDC_CRITIC_BLOCK, SDC_CRITIC_WAVES_PER_SIMD) sdc_critic_terminal_kernel(SdcCriticTerminal P) {
  __shared__ Lds L;
  passes(L, P.critic, P.rows, P.n_envs, [&](const long long env, const float v) {
    const double t = P.done[env] ? 0.0 : (double)v;
    P.score[env] = P.score[env] + P.factor * t;
  });
}

static unsigned critic_blocks(const long long n_rows) {
  const long long passes = (n_rows + SDC_CRITIC_BLOCK_ROWS - 1) / SDC_CRITIC_BLOCK_ROWS;
  return (unsigned)(passes < SDC_CRITIC_MAX_BLOCKS ? passes : SDC_CRITIC_MAX_BLOCKS);
}

hipError_t sdc_critic_values_launch(const SdcCriticValues& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_critic_values_kernel, dim3(critic_blocks(P.n_rows)), dim3(SDC_CRITIC_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_critic_terminal_launch(const SdcCriticTerminal& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_critic_terminal_kernel, dim3(critic_blocks(P.n_envs)), dim3(SDC_CRITIC_BLOCK), 0, st, P);
  return hipGetLastError();
}
