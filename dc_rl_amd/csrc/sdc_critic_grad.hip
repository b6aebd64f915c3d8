// sdc_critic_grad.hip -- sdc_critic_raw_kernel, sdc_value_loss_kernel, sdc_critic_grad_tanh_kernel / _relu_kernel,
// sdc_critic_grad_reduce_kernel and sdc_critic_grad_sq_kernel: the critic's raw output over rows of stored share_obs, the value loss
// and its derivative per row, and the gradient with respect to every parameter of the critic, for sdc_critic_evaluate, sdc_value_loss
// and sdc_critic_backward (sdc_capi.hip; the plans, the lane mappings, the order of every sum and the address bounds:
// sdc_critic_grad.hpp; the arithmetic: include/sustaindc_hip.h THE CRITIC'S GRADIENT).
//
// The networks are fp32 with nothing fused outside the matrix instructions and the forward's named fmaf (the library is built with
// -ffp-contract=off; the pragma below says it for this file whatever the flags); sdc_value_loss_kernel and the two reductions are fp64.
#include <hip/hip_runtime.h>

#include "sdc_critic.hpp"
#include "sdc_critic_grad.hpp"
#include "sdc_rowmlp.hpp"

#pragma clang fp contract(off)

namespace {

using sdc_act::f4;
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int WAVES = SDC_CRITIC_GRAD_BLOCK / 64;
constexpr int TILE_DW = sdc_rowmlp::TILE_DW<SDC_CRITIC_IN>;           // 464
constexpr int TILE_LOADS = sdc_rowmlp::TILE_LOADS<SDC_CRITIC_IN>;     // 8
constexpr int TILE_PAD = TILE_LOADS * 64;                     // 512: every lane of the gradient kernel stores all its eight dwords, the last 48 are fetch's zeros
constexpr int TT_DW = SDC_ROWMLP_H * SDC_ROWMLP_TS;           // a transposed tile: 64 units of 16 rows, 20 dwords apart
constexpr int TS = SDC_ROWMLP_TS;
constexpr int IN = SDC_CRITIC_IN, S1 = SDC_CRITIC_S1;
constexpr int N = SDC_CRITIC_N_PARAMS;
static_assert(4 * S1 == 32 && IN + 1 <= 32, "X's tile is 32 entries, and a padded one is free for the ONE");

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

struct Tiles {
  float obs[WAVES][TILE_PAD];
  float ta[WAVES][TT_DW];      // dZ^T
  float tb[WAVES][TT_DW];      // Y1^T (64 units), then X^T (the first 32)
};
struct alignas(16) Lds {      // (16-byte aligned: the A operands, the per-unit vectors and the tiles are read as 16-byte units)
  SdcCriticDev critic;
  SdcCriticGradDev critic_t;
  union {
    Tiles tile;
    float stage[N];            // the workgroup's sum, once the passes are over
  } u;
};
static_assert(sizeof(Lds) <= 160 * 1024, "one workgroup per CU");
static_assert(sizeof(Tiles) >= N * sizeof(float), "the stage lies inside the tiles");
static_assert(offsetof(Tiles, ta) % 16 == 0 && (TT_DW * sizeof(float)) % 16 == 0 && TS % 4 == 0, "a tile's 16-byte reads are aligned");
static_assert((SDC_CRITIC_GRAD_SQ_BLOCK & (SDC_CRITIC_GRAD_SQ_BLOCK - 1)) == 0, "the tree halves");

// what a lane fetches ahead for a pass: its eight dwords of the wavefront's share_obs tile and, for row e = lane & 15, the row's
// coefficient.  A row at or past n_rows is not loaded: zeros.
struct Fetched {
  float v[TILE_LOADS];
  float c;
};
__device__ __forceinline__ void fetch(Fetched& F, const SdcCriticGrad& P, const long long row0, const int lane) {
  const int valid = sdc_rowmlp::rows_that_exist(row0, P.n_rows);
  fetch_rows(F.v, P.rows, row0, P.n_rows, lane);
  const int e = lane & 15;
  F.c = 0.0f;
  if (e < valid) F.c = P.dvalue[row0 + e];
}

// the sums a wavefront keeps over all its passes
struct Acc {
  f4 w2[4][4];                 // [t][t']: register r = dW2[unit 16 t + 4 g + r][unit 16 t' + e]
  f4 w1[4][2];                 // [t][t']: register r = dW1[unit 16 t + 4 g + r][entry 16 t' + e]; entry 29 is a column of ones: db1
  f4 g1[4], be1[4];            // per-lane sums in the accumulators' layout: register (t, i) = unit 16 t + 4 g + i, this column's rows
  f4 b2[4], s2[4];             // s2 = sum_r c_r n2: dgain2, dW3 and (with db3) dbeta2 are its products, formed once
  float b3;
  float g0[S1], be0[S1];       // entry 4 s + g
};

// LayerNorm(64) backward from the forward's n and rs: dy -> dx = rs (dn - mean(dn) - n mean(dn n)), dn = dy gain
__device__ __forceinline__ void ln_dx(f4 (&d)[4], const f4 (&n)[4], const float rs, const float (&gain)[4][4][4], const int g) {
  f4 gn[4];
  sdc_rowmlp::unit_vector(gn, gain, g);
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float dn = d[t][i] * gn[t][i];
      d[t][i] = dn;
      s1 += dn;
      s2 += dn * n[t][i];
    }
  float sum, sq;
  sdc_rowmlp::all_sum2(s1, s2, sum, sq);
  const float m1 = sum * (1.0f / SDC_ROWMLP_H), m2 = sq * (1.0f / SDC_ROWMLP_H);
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) d[t][i] = rs * ((d[t][i] - m1) - n[t][i] * m2);
}

// a transposed tile (sdc_rowmlp::transpose_out stores it) back as an MFMA operand: rows 4 g .. 4 g + 3 of unit 16 t + e
__device__ __forceinline__ f4 transposed(const float* tile, const int t, const int g, const int e) {
  return *reinterpret_cast<const f4*>(tile + (16 * t + e) * TS + 4 * g);
}

// One pass of a wavefront over rows row0 .. row0 + 15: the trunk with a tape, the head's gradient, the backward.  F: what was fetched
// for this pass; on return what was fetched for the next (next0; past the grid's last pass nothing is loaded).
template <int KIND>
__device__ __forceinline__ void pass(Lds& L, Acc& A, Fetched& F, const SdcCriticGrad& P, const long long next0, const int wave, const int lane) {
  const int g = lane >> 4, e = lane & 15;
  float* const ta = L.u.tile.ta[wave];
  float* const tb = L.u.tile.tb[wave];
  // (no bound test on the tile's stores: every lane stores all its eight dwords, dwords 464 .. 511 are fetch's zeros)
#pragma unroll
  for (int j = 0; j < TILE_LOADS; j++) L.u.tile.obs[wave][lane + 64 * j] = F.v[j];
  __syncthreads();
  // entry 4 s + g of row e; entries 29 .. 31 (s = 7, g >= 1) are padding: what is read there (< 512) is dropped
  float x[S1];
#pragma unroll
  for (int s = 0; s < S1; s++) x[s] = L.u.tile.obs[wave][e * IN + 4 * s + g];
  x[S1 - 1] = g < 1 ? x[S1 - 1] : 0.0f;
  const float c = F.c;
  fetch(F, P, next0, lane);
  const SdcCriticDev* const W = &L.critic;
  sdc_rowmlp::Tape<S1> T;
  T.y1t = tb;
  f4 y2[4];
  sdc_rowmlp::trunk<KIND, SDC_CRITIC_IN>(W, x, lane, y2, T);

  // ---- the head: u = w3 . y2 + b3, dL/du = c: db3 += c, dy2 = w3 c, S += c n2 (dgain2, dbeta2 and dW3 are its products: emit) ---------
  A.b3 = A.b3 + c;
  f4 d[4];
  sdc_rowmlp::unit_vector(d, W->w3, g);
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      d[t][i] = d[t][i] * c;
      A.s2[t][i] = A.s2[t][i] + c * T.l2.n[t][i];
    }
  // ---- LayerNorm 2, activation 2: d = dZ2 ---------------------------------------------------------------------------------------------
  ln_dx(d, T.l2.n, T.l2.rs, W->ln2_g, g);
#pragma unroll
  for (int t = 0; t < 4; t++) {
    d[t] = d[t] * T.l2.dact[t];
    A.b2[t] = A.b2[t] + d[t];
  }
  // ---- dW2 += dZ2 Y1^T (Y1^T: the forward left it in tb): through the wavefront's tiles, rows on the k side ----------------------------
  sdc_rowmlp::transpose_out(ta, d, g, e);
  __syncthreads();
  {
    f4 a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
      a[t] = transposed(ta, t, g, e);
      b[t] = transposed(tb, t, g, e);
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int tp = 0; tp < 4; tp++) A.w2[t][tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][q], b[tp][q], A.w2[t][tp], 0, 0, 0);
  }
  // ---- dY1 = W2^T dZ2: dZ2 as it stands is the B operand of k-step s = 4 t + i --------------------------------------------------------
  f4 d1[4];
#pragma unroll
  for (int t = 0; t < 4; t++) d1[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < SDC_ROWMLP_S2; s++) {
    const f4 a = *reinterpret_cast<const f4*>(L.critic_t.a2t[s][lane]);
#pragma unroll
    for (int t = 0; t < 4; t++) d1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], d[s >> 2][s & 3], d1[t], 0, 0, 0);
  }
  // ---- LayerNorm 1 (its gain's and bias's sums), activation 1: d1 = dZ1 ---------------------------------------------------------------
#pragma unroll
  for (int t = 0; t < 4; t++) {
    A.g1[t] = A.g1[t] + d1[t] * T.l1.n[t];
    A.be1[t] = A.be1[t] + d1[t];
  }
  ln_dx(d1, T.l1.n, T.l1.rs, W->ln1_g, g);
#pragma unroll
  for (int t = 0; t < 4; t++) d1[t] = d1[t] * T.l1.dact[t];
  // ---- dW1 += dZ1 X^T (X: layer 1's input, 29 entries, then a ONE -- its column of dW1 is db1 -- and two zeros) -------------------------
  sdc_rowmlp::transpose_out(ta, d1, g, e);
#pragma unroll
  for (int s = 0; s < S1 - 1; s++) tb[(4 * s + g) * TS + e] = x[s];
  tb[(4 * (S1 - 1) + g) * TS + e] = g == 1 ? 1.0f : x[S1 - 1];      // (entry 28: x; 29: the one; 30, 31: x's zeros)
  __syncthreads();
  {
    f4 a[4], b[2];
#pragma unroll
    for (int t = 0; t < 4; t++) a[t] = transposed(ta, t, g, e);
#pragma unroll
    for (int tp = 0; tp < 2; tp++) b[tp] = transposed(tb, tp, g, e);
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int t = 0; t < 4; t++)
#pragma unroll
        for (int tp = 0; tp < 2; tp++) A.w1[t][tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][q], b[tp][q], A.w1[t][tp], 0, 0, 0);
  }
  // ---- the feature LayerNorm's gain and bias: dX = W1^T dZ1, register (t', r) = entry 4 (4 t' + r) + g ----------------------------------
  if (__builtin_amdgcn_readfirstlane(W->flags & 1)) {
    f4 dx[2];
    dx[0] = dx[1] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < SDC_ROWMLP_S2; s++) {
      const f2 a = *reinterpret_cast<const f2*>(L.critic_t.a1t[s][lane]);
#pragma unroll
      for (int tp = 0; tp < 2; tp++) dx[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tp], d1[s >> 2][s & 3], dx[tp], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < S1; s++) {
      const float v = dx[s >> 2][s & 3];
      A.g0[s] = A.g0[s] + v * T.l0.n[s];
      A.be0[s] = A.be0[s] + v;
    }
  }
}

// the sixteen columns' sums of one value, in every lane of the lane group: a butterfly, xor 1, 2, 4, 8
__device__ __forceinline__ float col_sum(float v) {
  v = v + __shfl_xor(v, 1, 64);
  v = v + __shfl_xor(v, 2, 64);
  v = v + __shfl_xor(v, 4, 64);
  v = v + __shfl_xor(v, 8, 64);
  return v;
}
__device__ __forceinline__ void col_sum(f4 (&v)[4]) {
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) v[t][i] = col_sum(v[t][i]);
}

// a wavefront's sums into the workgroup's stage: the first wavefront stores, the others add (each parameter has ONE lane per wavefront)
template <bool FIRST>
__device__ __forceinline__ void put(float* stage, const int j, const float v) {
  if (FIRST) stage[j] = v;
  else stage[j] = stage[j] + v;
}
template <bool FIRST>
__device__ __forceinline__ void emit(float* stage, const Acc& A, const SdcCriticDev& W, const int lane) {
  const int g = lane >> 4, e = lane & 15;
  // register r of tile t: unit 16 t + 4 g + r
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int unit = 16 * t + 4 * g + r;
#pragma unroll
      for (int tp = 0; tp < 4; tp++) put<FIRST>(stage, SDC_CGR_W2 + unit * SDC_ROWMLP_H + 16 * tp + e, A.w2[t][tp][r]);
      put<FIRST>(stage, SDC_CGR_W1 + unit * IN + e, A.w1[t][0][r]);
    }
  if (e < IN - 16) {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) put<FIRST>(stage, SDC_CGR_W1 + (16 * t + 4 * g + r) * IN + 16 + e, A.w1[t][1][r]);
  }
  if (e == IN - 16) {      // (the column of ones)
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) put<FIRST>(stage, SDC_CGR_B1 + 16 * t + 4 * g + r, A.w1[t][1][r]);
  }
  if (e == 0) {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int unit = 16 * t + 4 * g + r;
        const float S = A.s2[t][r], w3 = W.w3[g][t][r];
        put<FIRST>(stage, SDC_CGR_LN1G + unit, A.g1[t][r]);
        put<FIRST>(stage, SDC_CGR_LN1B + unit, A.be1[t][r]);
        put<FIRST>(stage, SDC_CGR_B2 + unit, A.b2[t][r]);
        // the head's three products of this wavefront's rows: dgain2 = w3 S, dbeta2 = w3 db3, dW3 = gain2 S + beta2 db3
        put<FIRST>(stage, SDC_CGR_LN2G + unit, w3 * S);
        put<FIRST>(stage, SDC_CGR_LN2B + unit, w3 * A.b3);
        put<FIRST>(stage, SDC_CGR_W3 + unit, W.ln2_g[g][t][r] * S + W.ln2_b[g][t][r] * A.b3);
      }
#pragma unroll
    for (int s = 0; s < S1; s++) {
      const int k = 4 * s + g;
      if (k < IN) {
        put<FIRST>(stage, SDC_CGR_LN0G + k, A.g0[s]);
        put<FIRST>(stage, SDC_CGR_LN0B + k, A.be0[s]);
      }
    }
  }
  if (lane == 0) put<FIRST>(stage, SDC_CGR_B3, A.b3);
}

template <int KIND>
__device__ __forceinline__ void grad_body(Lds& L, const SdcCriticGrad& P) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  Acc A;
  {
    const f4 zero = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
      for (int tp = 0; tp < 4; tp++) A.w2[t][tp] = zero;
      A.w1[t][0] = A.w1[t][1] = zero;
      A.g1[t] = A.be1[t] = A.b2[t] = A.s2[t] = zero;
    }
    A.b3 = 0.0f;
#pragma unroll
    for (int s = 0; s < S1; s++) A.g0[s] = A.be0[s] = 0.0f;
  }
  const long long n_pass = (P.n_rows + SDC_CRITIC_GRAD_BLOCK_ROWS - 1) / SDC_CRITIC_GRAD_BLOCK_ROWS;
  const long long stride = (long long)gridDim.x * SDC_CRITIC_GRAD_BLOCK_ROWS;
  Fetched F;
  fetch(F, P, (long long)blockIdx.x * SDC_CRITIC_GRAD_BLOCK_ROWS + wave * SDC_ROWMLP_ROWS, lane);
#pragma unroll 1
  for (long long p = blockIdx.x; p < n_pass; p += gridDim.x) {
    const long long row0 = p * SDC_CRITIC_GRAD_BLOCK_ROWS + wave * SDC_ROWMLP_ROWS;
    pass<KIND>(L, A, F, P, row0 + stride, wave, lane);
  }

  // ---- the sixteen columns, then the four wavefronts in their order, then the workgroup's partial -----------------------------------
  col_sum(A.g1); col_sum(A.be1); col_sum(A.b2); col_sum(A.s2);
  A.b3 = col_sum(A.b3);
#pragma unroll
  for (int s = 0; s < S1; s++) {
    A.g0[s] = col_sum(A.g0[s]);
    A.be0[s] = col_sum(A.be0[s]);
  }
  __syncthreads();      // (the stage lies inside the tiles: every wavefront is through with them)
  if (wave == 0) emit<true>(L.u.stage, A, L.critic, lane);
  __syncthreads();
#pragma unroll 1
  for (int w = 1; w < WAVES; w++) {
    if (wave == w) emit<false>(L.u.stage, A, L.critic, lane);
    __syncthreads();
  }
  float* const out = P.part + (size_t)blockIdx.x * N;
  for (int j = (int)threadIdx.x; j < N; j += SDC_CRITIC_GRAD_BLOCK) out[j] = L.u.stage[j];
}

}  // namespace

// (the activation is a template parameter, as the forward's, and here a kernel each: one body's registers are all a launch pays for)
extern "C" __global__ void __launch_bounds__(SDC_CRITIC_GRAD_BLOCK, 1) sdc_critic_grad_tanh_kernel(SdcCriticGrad P) {
  __shared__ Lds L;
  sdc_rowmlp::to_lds(&L.critic, P.critic);
  sdc_rowmlp::to_lds(&L.critic_t, P.critic_t);
  grad_body<0>(L, P);      // (the first pass's barrier orders the copies before the reads)
}
extern "C" __global__ void __launch_bounds__(SDC_CRITIC_GRAD_BLOCK, 1) sdc_critic_grad_relu_kernel(SdcCriticGrad P) {
  __shared__ Lds L;
  sdc_rowmlp::to_lds(&L.critic, P.critic);
  sdc_rowmlp::to_lds(&L.critic_t, P.critic_t);
  grad_body<1>(L, P);
}

// a parameter's B partials in workgroup order, fp64, rounded once
extern "C" __global__ void __launch_bounds__(SDC_CRITIC_GRAD_BLOCK) sdc_critic_grad_reduce_kernel(SdcCriticGradReduce P) {
  const int j = (int)(blockIdx.x * SDC_CRITIC_GRAD_BLOCK + threadIdx.x);
  if (j >= N) return;
  double s = 0.0;
  for (int b = 0; b < P.n_part; b++) s = s + (double)P.part[(size_t)b * N + j];
  P.grads[j] = (float)s;
}

// the squares of the stored fp32 gradients, fp64: lane l takes parameters l, l + 256, ... in that order, then the halving tree
extern "C" __global__ void __launch_bounds__(SDC_CRITIC_GRAD_SQ_BLOCK) sdc_critic_grad_sq_kernel(SdcCriticGradSq P) {
  __shared__ double part[SDC_CRITIC_GRAD_SQ_BLOCK];
  const int l = (int)threadIdx.x;
  double s = 0.0;
  for (int j = l; j < N; j += SDC_CRITIC_GRAD_SQ_BLOCK) {
    const double v = (double)P.grads[j];
    s = s + v * v;
  }
  part[l] = s;
  __syncthreads();
  for (int half = SDC_CRITIC_GRAD_SQ_BLOCK / 2; half >= 1; half >>= 1) {
    if (l < half) part[l] = part[l] + part[l + half];
    __syncthreads();
  }
  if (l == 0) P.grad_sq[0] = part[0];
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
  const dim3 grid(sdc_critic_grad_blocks(P.n_rows)), block(SDC_CRITIC_GRAD_BLOCK);
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
