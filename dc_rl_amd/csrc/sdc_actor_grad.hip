// sdc_actor_grad.hip -- sdc_actor_grad_tanh_kernel / _relu_kernel, sdc_actor_grad_reduce_kernel, sdc_actor_grad_sq_kernel and sdc_ppo_dlogp_kernel: the
// gradient of one agent's actor loss with respect to every parameter over rows of stored observations, and the PPO loss's derivative
// per stored log-probability, for sdc_actor_backward and sdc_ppo_dlogp (sdc_capi.hip; the arithmetic: include/sustaindc_hip.h THE
// ACTORS' GRADIENT).  The backward pass, its driver and the two reductions' bodies are the row networks' shared ones
// (sdc_rowmlp_grad.hpp: the plan, the lane mapping, the order of every sum, the LDS bounds); this file holds the actors' HEAD under it
// (what is theirs and their arrays' address bounds: sdc_actor_grad.hpp), sdc_ppo_dlogp_kernel and the launchers.
//
// fp32 with nothing fused outside the matrix instructions and the forward's named fmaf (the library is built with -ffp-contract=off;
// the pragma below says it for this file whatever the flags); sdc_ppo_dlogp_kernel and the two reductions are fp64.
#include <hip/hip_runtime.h>

#include "sdc_actor_forward.hpp"
#include "sdc_actor_grad.hpp"
#include "sdc_rowmlp.hpp"
#include "sdc_rowmlp_grad.hpp"

#pragma clang fp contract(off)

namespace {

using sdc_act::f4;
using sdc_rowmlp_grad::TS;
using sdc_rowmlp_grad::TT_DW;
using sdc_rowmlp_grad::WAVES;

// The actors' head under the shared backward (sdc_rowmlp_grad.hpp says what a head gives): strided rows with an action and a dlogp,
// three logits, the softmax's gradient, dW3 as a matrix product through two tiles of its own.
struct Head {
  static constexpr int IN = SDC_AEV_IN, OUT = SDC_AEV_OUT;
  using Dev = SdcActorEvalDev;
  using Args = SdcActorGrad;
  using At = SdcRowMlpGradAt<IN, OUT>;
  struct Tiles : sdc_rowmlp_grad::Tiles<IN> {
    float tc[WAVES][TT_DW];      // Y2^T
    float tl[WAVES][4 * TS];     // the logits' gradient [c][row]
  };
  // what a lane fetches ahead for a pass: its seven dwords of the wavefront's observation tile (sdc_rowmlp::fetch) and, for
  // row e = lane & 15, the action and the log-probability's coefficient.  A row at or past n_rows is not loaded: zeros, action -1.
  struct Row {
    int action;
    float dlogp;
  };
  struct Fetched {
    float v[sdc_rowmlp::TILE_LOADS<IN>];
    Row row;
  };
  struct Acc {
    f4 w3[4];                    // [t]: register r = dW3[c = e][unit 16 t + 4 g + r] (columns e >= 3: zeros)
    f4 g2[4];                    // (LayerNorm 2's bias has no sum of its own: dbeta2 = W3^T db3, formed once from db3)
    float b3[OUT];
  };
  struct Out {
    float lg[OUT];
  };

  static __device__ __forceinline__ void fetch(Fetched& F, const Args& P, const long long row0, const int lane) {
    const int valid = sdc_rowmlp::rows_that_exist(row0, P.n_rows);
    sdc_rowmlp::fetch<IN>(F.v, P.obs, P.row_stride, row0, P.n_rows, lane);
    const int e = lane & 15;
    F.row.action = -1;
    F.row.dlogp = 0.0f;
    if (e < valid) {
      F.row.action = P.actions[(row0 + e) * P.action_stride];
      F.row.dlogp = P.dlogp[row0 + e];
    }
  }

  template <int KIND, class TAPE>
  static __device__ __forceinline__ void forward(const Dev* W, float (&x)[SDC_AEV_S1], const int lane, Out& out, TAPE& T) {
    sdc_aev::forward_kind<KIND>(W, x, lane, out.lg, T);
  }

  // the logits' gradient dl_c = dlogp (1[c = a] - p_c) - dent p_c (log p_c + H); db3, d = dy2 = W3^T dl; Y2^T and dl^T into the tiles
  static __device__ __forceinline__ void gradient(Tiles& tile, Acc& A, const Args& P, const Row& now, const Out& out, const sdc_aev::Tape& T,
                                                  const Dev* W, f4 (&d)[4], const long long row0, const int wave, const int lane) {
    const int g = lane >> 4, e = lane & 15;
    const float dent = (float)P.dent;
    const float (&lg)[OUT] = out.lg;
    const float m = fmaxf(fmaxf(lg[0], lg[1]), lg[2]);
    float z[OUT], ex[OUT], lp[OUT], p[OUT], dl[OUT];
#pragma unroll
    for (int c = 0; c < OUT; c++) {
      z[c] = lg[c] - m;
      ex[c] = expf(z[c]);
    }
    const float sum = (ex[0] + ex[1]) + ex[2];
    const float lse = logf(sum);
#pragma unroll
    for (int c = 0; c < OUT; c++) {
      lp[c] = z[c] - lse;
      p[c] = ex[c] / sum;
    }
    const float H = -((p[0] * lp[0] + p[1] * lp[1]) + p[2] * lp[2]);
#pragma unroll
    for (int c = 0; c < OUT; c++) {
      const float hot = now.action == c ? 1.0f : 0.0f;
      dl[c] = now.dlogp * (hot - p[c]) - dent * (p[c] * (lp[c] + H));
    }
    // (a row past n_rows: fetch gave it dlogp 0, but dent reaches every row -- its gradient is set to zero outright)
    if (row0 + e >= P.n_rows) {
#pragma unroll
      for (int c = 0; c < OUT; c++) dl[c] = 0.0f;
    }
#pragma unroll
    for (int t = 0; t < 4; t++) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < OUT; c++) {
      A.b3[c] = A.b3[c] + dl[c];
      f4 w3[4];
      sdc_rowmlp::unit_vector(w3, W->w3[c], g);
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) d[t][i] = d[t][i] + dl[c] * w3[t][i];
    }
    sdc_rowmlp::transpose_out(tile.tc[wave], T.y2, g, e);
    tile.tl[wave][g * TS + e] = g == 0 ? dl[0] : (g == 1 ? dl[1] : (g == 2 ? dl[2] : 0.0f));      // (row 3: zeros)
  }

  static __device__ __forceinline__ f4* ln2_gain(Acc& A) { return A.g2; }

  // dW3 += Y2 dl^T: rows on the k side, as dW2
  static __device__ __forceinline__ void products(const Tiles& tile, Acc& A, const int wave, const int lane) {
    const int g = lane >> 4, e = lane & 15;
    const f4 bl = *reinterpret_cast<const f4*>(tile.tl[wave] + (e < OUT ? e : OUT) * TS + 4 * g);      // B[row 4 g + q][c = e]; c >= 3: zeros
    f4 y[4];
#pragma unroll
    for (int t = 0; t < 4; t++) y[t] = sdc_rowmlp_grad::transposed(tile.tc[wave], t, g, e);
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int t = 0; t < 4; t++) A.w3[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(y[t][q], bl[q], A.w3[t], 0, 0, 0);
  }

  static __device__ __forceinline__ void col_sums(Acc& A) {
    sdc_rowmlp_grad::col_sum(A.g2);
#pragma unroll
    for (int c = 0; c < OUT; c++) A.b3[c] = sdc_rowmlp_grad::col_sum(A.b3[c]);
  }

  template <bool FIRST>
  static __device__ __forceinline__ void emit(float* stage, const Acc& A, const Dev& W, const int lane) {
    using sdc_rowmlp_grad::put;
    const int g = lane >> 4, e = lane & 15;
    if (e < OUT) {
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) put<FIRST>(stage, At::W3 + e * SDC_ROWMLP_H + 16 * t + 4 * g + r, A.w3[t][r]);
    }
    if (e == 0) {
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int unit = 16 * t + 4 * g + r;
          put<FIRST>(stage, At::LN2G + unit, A.g2[t][r]);
          // dbeta2 = W3^T db3 of this wavefront's rows
          put<FIRST>(stage, At::LN2B + unit, (W.w3[0][g][t][r] * A.b3[0] + W.w3[1][g][t][r] * A.b3[1]) + W.w3[2][g][t][r] * A.b3[2]);
        }
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < OUT; c++) put<FIRST>(stage, At::B3 + c, A.b3[c]);
    }
  }
};

using Lds = sdc_rowmlp_grad::Lds<Head>;
static_assert(sizeof(Lds) <= 160 * 1024, "one workgroup per CU");
constexpr int N = SDC_ACTOR_N_PARAMS;

}  // namespace

// (the activation is a template parameter, as the forward's, and here a kernel each: one body's registers are all a launch pays for)
extern "C" __global__ void __launch_bounds__(SDC_ACTOR_GRAD_BLOCK, 1) sdc_actor_grad_tanh_kernel(SdcActorGrad P) {
  __shared__ Lds L;
  sdc_rowmlp::to_lds(&L.net, P.actor);
  sdc_rowmlp::to_lds(&L.net_t, P.actor_t);
  sdc_rowmlp_grad::grad_body<0, Head>(L, P);
}
extern "C" __global__ void __launch_bounds__(SDC_ACTOR_GRAD_BLOCK, 1) sdc_actor_grad_relu_kernel(SdcActorGrad P) {
  __shared__ Lds L;
  sdc_rowmlp::to_lds(&L.net, P.actor);
  sdc_rowmlp::to_lds(&L.net_t, P.actor_t);
  sdc_rowmlp_grad::grad_body<1, Head>(L, P);
}

extern "C" __global__ void __launch_bounds__(SDC_ACTOR_GRAD_BLOCK) sdc_actor_grad_reduce_kernel(SdcActorGradReduce P) {
  sdc_rowmlp_grad::reduce<N>(P);
}
extern "C" __global__ void __launch_bounds__(SDC_ACTOR_GRAD_SQ_BLOCK) sdc_actor_grad_sq_kernel(SdcActorGradSq P) {
  sdc_rowmlp_grad::grad_sq<N, SDC_ACTOR_GRAD_SQ_BLOCK>(P);
}

// d(-scale sum F min(r A, clamp(r) A)) / d logp per element: sdc_ppo_terms_kernel's terms, in its words
extern "C" __global__ void __launch_bounds__(SDC_PPO_BLOCK) sdc_ppo_dlogp_kernel(SdcPpoDlogp P) {
  const long long stride = (long long)gridDim.x * SDC_PPO_BLOCK;
  const size_t col = (size_t)P.agent;
  for (long long i = (long long)blockIdx.x * SDC_PPO_BLOCK + threadIdx.x; i < P.n; i += stride) {
    const size_t j = (size_t)i * 3 + col;      // (the column is part of the address)
    const double lr = (double)P.new_lp[j] - (double)P.old_lp[j];
    const double r = exp(lr);
    const double A = (double)P.adv[i];
    float ff = 1.0f;
    if (P.factor) ff = P.factor[i];
    const double F = (double)ff;
    const double s1 = r * A;
    double rc = r < P.lo ? P.lo : r;
    rc = rc > P.hi ? P.hi : rc;
    const double s2 = rc * A;
    const bool clipped = r < P.lo || r > P.hi;
    const bool open = !clipped || s1 < s2;
    const double d = -(((P.scale * F) * A) * r);
    P.dlogp[i] = (float)(open ? d : 0.0);
  }
}

hipError_t sdc_actor_grad_launch(const SdcActorGrad& P, const int activation, hipStream_t st) {
  const dim3 grid(sdc_rowmlp_grad_blocks(P.n_rows, SDC_ACTOR_GRAD_MAX_BLOCKS)), block(SDC_ACTOR_GRAD_BLOCK);
  if (activation == 1) hipLaunchKernelGGL(sdc_actor_grad_relu_kernel, grid, block, 0, st, P);
  else hipLaunchKernelGGL(sdc_actor_grad_tanh_kernel, grid, block, 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_actor_grad_reduce_launch(const SdcActorGradReduce& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_actor_grad_reduce_kernel, dim3((N + SDC_ACTOR_GRAD_BLOCK - 1) / SDC_ACTOR_GRAD_BLOCK), dim3(SDC_ACTOR_GRAD_BLOCK), 0,
                     st, P);
  return hipGetLastError();
}

hipError_t sdc_actor_grad_sq_launch(const SdcActorGradSq& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_actor_grad_sq_kernel, dim3(1), dim3(SDC_ACTOR_GRAD_SQ_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_ppo_dlogp_launch(const SdcPpoDlogp& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_ppo_dlogp_kernel, dim3(sdc_ppo_blocks(P.n)), dim3(SDC_PPO_BLOCK), 0, st, P);
  return hipGetLastError();
}
