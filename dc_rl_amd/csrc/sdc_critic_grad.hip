// sdc_critic_grad.hip -- sdc_critic_raw_kernel, sdc_value_loss_kernel, sdc_critic_grad_tanh_kernel / _relu_kernel,
// sdc_critic_grad_reduce_kernel and sdc_critic_grad_sq_kernel: the critic's raw output over rows of stored share_obs, the value loss
// and its derivative per row, and the gradient with respect to every parameter of the critic, for sdc_critic_evaluate, sdc_value_loss
// and sdc_critic_backward (sdc_capi.hip; the plans and the address bounds: sdc_critic_grad.hpp; the arithmetic:
// include/sustaindc_hip.h THE CRITIC'S GRADIENT).  The backward pass, its driver and the two reductions' bodies are the row networks'
// shared ones (sdc_rowmlp_grad.hpp: the lane mapping, the order of every sum, the LDS bounds); this file holds the critic's HEAD under it.
//
// The networks are fp32 with nothing fused outside the matrix instructions and the forward's named fmaf (the library is built with
// -ffp-contract=off; the pragma below says it for this file whatever the flags); sdc_value_loss_kernel and the two reductions are fp64.
#include <hip/hip_runtime.h>

#include "sdc_critic.hpp"
#include "sdc_critic_grad.hpp"
#include "sdc_rowmlp.hpp"
#include "sdc_rowmlp_grad.hpp"

#pragma clang fp contract(off)

namespace {

using sdc_act::f4;

constexpr int TILE_DW = sdc_rowmlp::TILE_DW<SDC_CRITIC_IN>;           // 464
constexpr int TILE_LOADS = sdc_rowmlp::TILE_LOADS<SDC_CRITIC_IN>;     // 8
constexpr int IN = SDC_CRITIC_IN, S1 = SDC_CRITIC_S1;
constexpr int N = SDC_CRITIC_N_PARAMS;

// A wavefront's rows row0 .. row0 + 15 of `rows` (n_rows in all), densely: lane l takes dwords l, l + 64, ... of the 464; a dword of
// a row at or past n_rows is not loaded (0).  (sdc_critic.hip's fetch, in its words: that file keeps its source.)
__device__ __forceinline__ void fetch_rows(float (&v)[TILE_LOADS], const float* rows, const long long row0, const long long n_rows, const int lane) {
  const int valid = sdc_rowmlp::rows_that_exist(row0, n_rows) * IN;      // dwords that exist
  const float* const src = rows + row0 * IN;
#pragma unroll
  for (int j = 0; j < TILE_LOADS; j++) {
    const int u = lane + 64 * j;
    v[j] = 0.0f;
    if (u < valid) v[j] = src[u];
  }
}

// ---- the raw output -----------------------------------------------------------------------------------------------------------------
using RawLds = sdc_rowmlp::Lds<SdcCriticDev, SDC_CRITIC_IN>;
static_assert(sizeof(RawLds) <= 40 * 1024, "four workgroups' LDS fit a CU");

// sdc_critic::forward_kind's head up to the value it scales: the same operations in the same order, so that
// sdc_critic_values = (u * scale) + shift to the bit
template <int KIND>
__device__ __forceinline__ float raw_kind(const SdcCriticDev* W, float (&x)[S1], const int lane) {
  sdc_rowmlp::NoTape none;
  f4 acc[4];
  sdc_rowmlp::trunk<KIND, SDC_CRITIC_IN>(W, x, lane, acc, none);
  const float v = sdc_rowmlp::unit_dot(W->w3, acc, lane >> 4);
  return sdc_rowmlp::all_sum(v) + W->b3;
}

// One pass of a wavefront (sdc_critic.hip's pass): the fetched dwords through the wavefront's tile -> u of row (lane & 15)
__device__ __forceinline__ float raw_pass(RawLds& L, float (&v)[TILE_LOADS], const float* rows, const long long next0, const long long n_rows,
                                          const int wave, const int lane) {
#pragma unroll
  for (int j = 0; j < TILE_LOADS; j++) {
    const int u = lane + 64 * j;
    if (u < TILE_DW) L.tile[wave][u] = v[j];
  }
  __syncthreads();
  const int g = lane >> 4, e = lane & 15;
  float x[S1];
#pragma unroll
  for (int s = 0; s < S1; s++) {
    const int k = 4 * s + g;
    x[s] = 0.0f;
    if (k < IN) x[s] = L.tile[wave][e * IN + k];
  }
  fetch_rows(v, rows, next0, n_rows, lane);
  if (__builtin_amdgcn_readfirstlane((L.net.flags >> 1) & 3) == 1) return raw_kind<1>(&L.net, x, lane);
  return raw_kind<0>(&L.net, x, lane);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_CRITIC_BLOCK, SDC_CRITIC_WAVES_PER_SIMD) sdc_critic_raw_kernel(SdcCriticRaw P) {
  __shared__ RawLds L;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  sdc_rowmlp::to_lds(&L.net, P.critic);
  const long long n_pass = (P.n_rows + SDC_CRITIC_BLOCK_ROWS - 1) / SDC_CRITIC_BLOCK_ROWS;
  const long long stride = (long long)gridDim.x * SDC_CRITIC_BLOCK_ROWS;
  long long row0 = (long long)blockIdx.x * SDC_CRITIC_BLOCK_ROWS + wave * SDC_ROWMLP_ROWS;
  float v[TILE_LOADS];
  fetch_rows(v, P.rows, row0, P.n_rows, lane);
#pragma unroll 1
  for (long long p = blockIdx.x; p < n_pass; p += gridDim.x, row0 += stride) {
    // (a next pass that does not exist starts at or past n_rows -- the grid's stride is whole workgroups --: fetch loads nothing)
    const float u = raw_pass(L, v, P.rows, row0 + stride, P.n_rows, wave, lane);
    const long long row = row0 + lane;
    if (lane < SDC_ROWMLP_ROWS && row < P.n_rows) P.raw[row] = u;
  }
}

// ---- the value loss -----------------------------------------------------------------------------------------------------------------
// (the pass and its fold: sdc_value_loss_dev.hpp, shared with sdc_minibatch.hip's sdc_value_loss_normed_kernel)
#include "sdc_value_loss_dev.hpp"

extern "C" __global__ void __launch_bounds__(SDC_PPO_BLOCK) sdc_value_loss_kernel(SdcValueLoss P) {
  __shared__ double part[7][SDC_PPO_BLOCK];
  // (the switches are the launch's, the same in every lane: the barriers of the statistics are reached by all or by none)
  const bool huber = (P.flags & SDC_VALUE_LOSS_HUBER) != 0;
  if (P.part) {
    if (huber) value_loss_pass<true, true>(P, part);
    else value_loss_pass<false, true>(P, part);
  } else {
    if (huber) value_loss_pass<true, false>(P, part);
    else value_loss_pass<false, false>(P, part);
  }
}

// ---- the gradient -------------------------------------------------------------------------------------------------------------------
namespace {

// The critic's head under the shared backward (sdc_rowmlp_grad.hpp says what a head gives): dense rows with a coefficient c =
// dvalue[row], one output u = w3 . y2 + b3, so dy2 = w3 c, db3 = sum c, and dgain2, dbeta2 and dW3 are products of the ONE per-lane sum
// S = sum_r c_r n2, formed at the end (sdc_critic_grad.hpp says why).
struct Head {
  static constexpr int IN = SDC_CRITIC_IN, OUT = 1;
  using Dev = SdcCriticDev;
  using Args = SdcCriticGrad;
  using At = SdcRowMlpGradAt<IN, OUT>;
  using Tiles = sdc_rowmlp_grad::Tiles<IN>;
  // what a lane fetches ahead for a pass: its eight dwords of the wavefront's share_obs tile and, for row e = lane & 15, the row's
  // coefficient.  A row at or past n_rows is not loaded: zeros.
  struct Row {
    float c;
  };
  struct Fetched {
    float v[TILE_LOADS];
    Row row;
  };
  struct Acc {
    f4 s2[4];                    // S
    float b3;
  };
  struct Out {
    f4 y2[4];
  };

  static __device__ __forceinline__ void fetch(Fetched& F, const Args& P, const long long row0, const int lane) {
    const int valid = sdc_rowmlp::rows_that_exist(row0, P.n_rows);
    fetch_rows(F.v, P.rows, row0, P.n_rows, lane);
    const int e = lane & 15;
    F.row.c = 0.0f;
    if (e < valid) F.row.c = P.dvalue[row0 + e];
  }

  template <int KIND, class TAPE>
  static __device__ __forceinline__ void forward(const Dev* W, float (&x)[S1], const int lane, Out& out, TAPE& T) {
    sdc_rowmlp::trunk<KIND, SDC_CRITIC_IN>(W, x, lane, out.y2, T);
  }

  static __device__ __forceinline__ void gradient(Tiles&, Acc& A, const Args&, const Row& now, const Out&, const sdc_rowmlp::Tape<S1>& T,
                                                  const Dev* W, f4 (&d)[4], const long long, const int, const int lane) {
    const float c = now.c;
    A.b3 = A.b3 + c;
    sdc_rowmlp::unit_vector(d, W->w3, lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int i = 0; i < 4; i++) {
        d[t][i] = d[t][i] * c;
        A.s2[t][i] = A.s2[t][i] + c * T.l2.n[t][i];
      }
  }

  static __device__ __forceinline__ f4* ln2_gain(Acc&) { return nullptr; }
  static __device__ __forceinline__ void products(const Tiles&, Acc&, const int, const int) {}

  static __device__ __forceinline__ void col_sums(Acc& A) {
    sdc_rowmlp_grad::col_sum(A.s2);
    A.b3 = sdc_rowmlp_grad::col_sum(A.b3);
  }

  template <bool FIRST>
  static __device__ __forceinline__ void emit(float* stage, const Acc& A, const Dev& W, const int lane) {
    using sdc_rowmlp_grad::put;
    const int g = lane >> 4, e = lane & 15;
    if (e == 0) {
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int unit = 16 * t + 4 * g + r;
          const float S = A.s2[t][r], w3 = W.w3[g][t][r];
          // the head's three products of this wavefront's rows: dgain2 = w3 S, dbeta2 = w3 db3, dW3 = gain2 S + beta2 db3
          put<FIRST>(stage, At::LN2G + unit, w3 * S);
          put<FIRST>(stage, At::LN2B + unit, w3 * A.b3);
          put<FIRST>(stage, At::W3 + unit, W.ln2_g[g][t][r] * S + W.ln2_b[g][t][r] * A.b3);
        }
    }
    if (lane == 0) put<FIRST>(stage, At::B3, A.b3);
  }
};

using Lds = sdc_rowmlp_grad::Lds<Head>;
static_assert(sizeof(Lds) <= 160 * 1024, "one workgroup per CU");

}  // namespace

// (the activation is a template parameter, as the forward's, and here a kernel each: one body's registers are all a launch pays for)
extern "C" __global__ void __launch_bounds__(SDC_CRITIC_GRAD_BLOCK, 1) sdc_critic_grad_tanh_kernel(SdcCriticGrad P) {
  __shared__ Lds L;
  sdc_rowmlp::to_lds(&L.net, P.critic);
  sdc_rowmlp::to_lds(&L.net_t, P.critic_t);
  sdc_rowmlp_grad::grad_body<0, Head>(L, P);
}
extern "C" __global__ void __launch_bounds__(SDC_CRITIC_GRAD_BLOCK, 1) sdc_critic_grad_relu_kernel(SdcCriticGrad P) {
  __shared__ Lds L;
  sdc_rowmlp::to_lds(&L.net, P.critic);
  sdc_rowmlp::to_lds(&L.net_t, P.critic_t);
  sdc_rowmlp_grad::grad_body<1, Head>(L, P);
}

extern "C" __global__ void __launch_bounds__(SDC_CRITIC_GRAD_BLOCK) sdc_critic_grad_reduce_kernel(SdcCriticGradReduce P) {
  sdc_rowmlp_grad::reduce<N>(P);
}
extern "C" __global__ void __launch_bounds__(SDC_CRITIC_GRAD_SQ_BLOCK) sdc_critic_grad_sq_kernel(SdcCriticGradSq P) {
  sdc_rowmlp_grad::grad_sq<N, SDC_CRITIC_GRAD_SQ_BLOCK>(P);
}

static unsigned raw_blocks(const long long n_rows) {
  const long long passes = (n_rows + SDC_CRITIC_BLOCK_ROWS - 1) / SDC_CRITIC_BLOCK_ROWS;
  return (unsigned)(passes < SDC_CRITIC_MAX_BLOCKS ? passes : SDC_CRITIC_MAX_BLOCKS);
}

hipError_t sdc_critic_raw_launch(const SdcCriticRaw& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_critic_raw_kernel, dim3(raw_blocks(P.n_rows)), dim3(SDC_CRITIC_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_value_loss_launch(const SdcValueLoss& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_value_loss_kernel, dim3(sdc_ppo_blocks(P.n)), dim3(SDC_PPO_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_critic_grad_launch(const SdcCriticGrad& P, const int activation, hipStream_t st) {
  const dim3 grid(sdc_rowmlp_grad_blocks(P.n_rows, SDC_CRITIC_GRAD_MAX_BLOCKS)), block(SDC_CRITIC_GRAD_BLOCK);
  if (activation == 1) hipLaunchKernelGGL(sdc_critic_grad_relu_kernel, grid, block, 0, st, P);
  else hipLaunchKernelGGL(sdc_critic_grad_tanh_kernel, grid, block, 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_critic_grad_reduce_launch(const SdcCriticGradReduce& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_critic_grad_reduce_kernel, dim3((N + SDC_CRITIC_GRAD_BLOCK - 1) / SDC_CRITIC_GRAD_BLOCK), dim3(SDC_CRITIC_GRAD_BLOCK), 0,
                     st, P);
  return hipGetLastError();
}

hipError_t sdc_critic_grad_sq_launch(const SdcCriticGradSq& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_critic_grad_sq_kernel, dim3(1), dim3(SDC_CRITIC_GRAD_SQ_BLOCK), 0, st, P);
  return hipGetLastError();
}
