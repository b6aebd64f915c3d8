// sdc_actor_grad.hip -- sdc_actor_grad_tanh_kernel / _relu_kernel, sdc_actor_grad_reduce_kernel, sdc_actor_grad_sq_kernel and sdc_ppo_dlogp_kernel: the
// gradient of one agent's actor loss with respect to every parameter over rows of stored observations, and the PPO loss's derivative
// per stored log-probability, for sdc_actor_backward and sdc_ppo_dlogp (sdc_capi.hip; the plans, the lane mappings, the order of every
// sum and the address bounds: sdc_actor_grad.hpp; the arithmetic: include/sustaindc_hip.h THE ACTORS' GRADIENT).
//
// fp32 with nothing fused outside the matrix instructions and the forward's named fmaf (the library is built with -ffp-contract=off;
// the pragma below says it for this file whatever the flags); sdc_ppo_dlogp_kernel and the two reductions are fp64.
#include <hip/hip_runtime.h>

#include "sdc_actor_forward.hpp"
#include "sdc_actor_grad.hpp"
#include "sdc_rowmlp.hpp"

#pragma clang fp contract(off)

namespace {

using sdc_act::f4;
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int WAVES = SDC_ACTOR_GRAD_BLOCK / 64;
constexpr int TILE_LOADS = sdc_rowmlp::TILE_LOADS<SDC_AEV_IN>;        // 7
constexpr int TILE_PAD = TILE_LOADS * 64;                     // 448: every lane stores all its seven dwords, the last 32 are never read
constexpr int TT_DW = SDC_ROWMLP_H * SDC_AGR_S;               // a transposed tile: 64 units of 16 rows, 20 dwords apart
constexpr int N = SDC_ACTOR_N_PARAMS;

struct Tiles {
  float obs[WAVES][TILE_PAD];
  float ta[WAVES][TT_DW];      // dZ^T
  float tb[WAVES][TT_DW];      // Y1^T (64 units), then X^T (the first 32)
  float tc[WAVES][TT_DW];      // Y2^T
  float tl[WAVES][4 * SDC_AGR_S];      // the logits' gradient [c][row]
};
struct alignas(16) Lds {      // (16-byte aligned: the A operands, the per-unit vectors and the tiles are read as 16-byte units)
  SdcActorEvalDev actor;
  SdcActorGradDev actor_t;
  union {
    Tiles tile;
    float stage[N];            // the workgroup's sum, once the passes are over
  } u;
};
static_assert(sizeof(Lds) <= 160 * 1024, "one workgroup per CU");
static_assert(sizeof(Tiles) >= N * sizeof(float), "the stage lies inside the tiles");
static_assert(offsetof(Tiles, ta) % 16 == 0 && (TT_DW * sizeof(float)) % 16 == 0 && SDC_AGR_S % 4 == 0, "a tile's 16-byte reads are aligned");
static_assert((SDC_ACTOR_GRAD_SQ_BLOCK & (SDC_ACTOR_GRAD_SQ_BLOCK - 1)) == 0, "the tree halves");

// what a lane fetches ahead for a pass: its seven dwords of the wavefront's observation tile (sdc_rowmlp::fetch) and, for
// row e = lane & 15, the action and the log-probability's coefficient.  A row at or past n_rows is not loaded: zeros, action -1.
struct Fetched {
  float v[TILE_LOADS];
  int action;
  float dlogp;
};
__device__ __forceinline__ void fetch(Fetched& F, const SdcActorGrad& P, const long long row0, const int lane) {
  const int valid = sdc_rowmlp::rows_that_exist(row0, P.n_rows);
  sdc_rowmlp::fetch<SDC_AEV_IN>(F.v, P.obs, P.row_stride, row0, P.n_rows, lane);
  const int e = lane & 15;
  F.action = -1;
  F.dlogp = 0.0f;
  if (e < valid) {
    F.action = P.actions[(row0 + e) * P.action_stride];
    F.dlogp = P.dlogp[row0 + e];
  }
}

// the sums a wavefront keeps over all its passes
struct Acc {
  f4 w2[4][4];                 // [t][t']: register r = dW2[unit 16 t + 4 g + r][unit 16 t' + e]
  f4 w1[4][2];                 // [t][t']: register r = dW1[unit 16 t + 4 g + r][entry 16 t' + e]; entry 26 is a column of ones: db1
  f4 w3[4];                    // [t]: register r = dW3[c = e][unit 16 t + 4 g + r] (columns e >= 3: zeros)
  f4 g1[4], be1[4];            // per-lane sums in the accumulators' layout: register (t, i) = unit 16 t + 4 g + i, this column's rows
  f4 b2[4], g2[4];             // (LayerNorm 2's bias has no sum of its own: dbeta2 = W3^T db3, formed once from db3)
  float b3[SDC_AEV_OUT];
  float g0[SDC_AEV_S1], be0[SDC_AEV_S1];      // entry 4 s + g
};

// LayerNorm(64) backward from the forward's n and rs: the gain's and the bias's sums, dy -> dx = rs (dn - mean(dn) - n mean(dn n))
__device__ __forceinline__ void ln_back(f4 (&d)[4], const f4 (&n)[4], const float rs, const float (&gain)[4][4][4], const int g,
                                        f4 (&dgain)[4], f4* const dbias) {
  f4 gn[4];
  sdc_rowmlp::unit_vector(gn, gain, g);
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float dy = d[t][i];
      dgain[t][i] = dgain[t][i] + dy * n[t][i];
      if (dbias) dbias[t][i] = dbias[t][i] + dy;
      const float dn = dy * gn[t][i];
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

// dx -> dz = dx act'(z), added to the layer bias's sums
__device__ __forceinline__ void act_back(f4 (&d)[4], const f4 (&dact)[4], f4 (&dbias)[4]) {
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      d[t][i] = d[t][i] * dact[t][i];
      dbias[t][i] = dbias[t][i] + d[t][i];
    }
}

// a transposed tile (sdc_rowmlp::transpose_out stores it) back as an MFMA operand: rows 4 g .. 4 g + 3 of unit 16 t + e
__device__ __forceinline__ f4 transposed(const float* tile, const int t, const int g, const int e) {
  return *reinterpret_cast<const f4*>(tile + (16 * t + e) * SDC_AGR_S + 4 * g);
}

// One pass of a wavefront over rows row0 .. row0 + 15: forward with a tape, the logits' gradient, the backward.  F: what was fetched for
// this pass; on return what was fetched for the next (next0; past the grid's last pass nothing is loaded).
template <int KIND>
__device__ __forceinline__ void pass(Lds& L, Acc& A, Fetched& F, const SdcActorGrad& P, const float dent, const long long row0,
                                     const long long next0, const int wave, const int lane) {
  const int g = lane >> 4, e = lane & 15;
  float* const ta = L.u.tile.ta[wave];
  float* const tb = L.u.tile.tb[wave];
  float* const tc = L.u.tile.tc[wave];
  float* const tl = L.u.tile.tl[wave];
  // (not the critic's and evaluate's store and pick with their bound tests: a lane predicate costs an SGPR pair this kernel does not
  // have -- the tile is padded instead, every lane stores all its seven dwords, dwords 416 .. 447 fetch's zeros)
#pragma unroll
  for (int j = 0; j < TILE_LOADS; j++) L.u.tile.obs[wave][lane + 64 * j] = F.v[j];
  __syncthreads();
  // entry 4 s + g of row e; entries 26, 27 (s = 6, g >= 2) are padding: what is read there (< 448) is dropped
  float x[SDC_AEV_S1];
#pragma unroll
  for (int s = 0; s < SDC_AEV_S1; s++) x[s] = L.u.tile.obs[wave][e * SDC_AEV_IN + 4 * s + g];
  x[SDC_AEV_S1 - 1] = g < 2 ? x[SDC_AEV_S1 - 1] : 0.0f;
  const int action = F.action;
  const float dlp = F.dlogp;
  fetch(F, P, next0, lane);
  const SdcActorEvalDev* const W = &L.actor;
  sdc_aev::Tape T;
  T.y1t = tb;
  float lg[SDC_AEV_OUT];
  sdc_aev::forward_kind<KIND>(W, x, lane, lg, T);

  // ---- the logits' gradient: dl_c = dlogp (1[c = a] - p_c) - dent p_c (log p_c + H) ---------------------------------------------------
  const float m = fmaxf(fmaxf(lg[0], lg[1]), lg[2]);
  float z[SDC_AEV_OUT], ex[SDC_AEV_OUT], lp[SDC_AEV_OUT], p[SDC_AEV_OUT], dl[SDC_AEV_OUT];
#pragma unroll
  for (int c = 0; c < SDC_AEV_OUT; c++) {
    z[c] = lg[c] - m;
    ex[c] = expf(z[c]);
  }
  const float sum = (ex[0] + ex[1]) + ex[2];
  const float lse = logf(sum);
#pragma unroll
  for (int c = 0; c < SDC_AEV_OUT; c++) {
    lp[c] = z[c] - lse;
    p[c] = ex[c] / sum;
  }
  const float H = -((p[0] * lp[0] + p[1] * lp[1]) + p[2] * lp[2]);
#pragma unroll
  for (int c = 0; c < SDC_AEV_OUT; c++) {
    const float hot = action == c ? 1.0f : 0.0f;
    dl[c] = dlp * (hot - p[c]) - dent * (p[c] * (lp[c] + H));
  }
  // (a row past n_rows: fetch gave it dlogp 0, but dent reaches every row -- its gradient is set to zero outright)
  if (row0 + e >= P.n_rows) {
#pragma unroll
    for (int c = 0; c < SDC_AEV_OUT; c++) dl[c] = 0.0f;
  }

  // ---- the last layer: db3, dy2 = W3^T dl; dW3 += dl Y2^T rides the tiles below --------------------------------------------------------
  f4 d[4];
#pragma unroll
  for (int t = 0; t < 4; t++) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < SDC_AEV_OUT; c++) {
    A.b3[c] = A.b3[c] + dl[c];
    f4 w3[4];
    sdc_rowmlp::unit_vector(w3, W->w3[c], g);
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int i = 0; i < 4; i++) d[t][i] = d[t][i] + dl[c] * w3[t][i];
  }
  sdc_rowmlp::transpose_out(tc, T.y2, g, e);
  tl[g * SDC_AGR_S + e] = g == 0 ? dl[0] : (g == 1 ? dl[1] : (g == 2 ? dl[2] : 0.0f));      // (row 3: zeros)
  // ---- LayerNorm 2, activation 2: d = dZ2 ---------------------------------------------------------------------------------------------
  ln_back(d, T.l2.n, T.l2.rs, W->ln2_g, g, A.g2, nullptr);
  act_back(d, T.l2.dact, A.b2);
  // ---- dW2 += dZ2 Y1^T (Y1^T: the forward left it in tb), dW3 += Y2 dl^T: through the wavefront's tiles, rows on the k side ------------
  sdc_rowmlp::transpose_out(ta, d, g, e);
  __syncthreads();
  {
    f4 a[4], b[4], y[4];
    const f4 bl = *reinterpret_cast<const f4*>(tl + (e < SDC_AEV_OUT ? e : SDC_AEV_OUT) * SDC_AGR_S + 4 * g);      // B[row 4 g + q][c = e]; c >= 3: zeros
#pragma unroll
    for (int t = 0; t < 4; t++) {
      a[t] = transposed(ta, t, g, e);
      b[t] = transposed(tb, t, g, e);
      y[t] = transposed(tc, t, g, e);
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int tp = 0; tp < 4; tp++) A.w2[t][tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][q], b[tp][q], A.w2[t][tp], 0, 0, 0);
        A.w3[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(y[t][q], bl[q], A.w3[t], 0, 0, 0);
      }
  }
  // ---- dY1 = W2^T dZ2: dZ2 as it stands is the B operand of k-step s = 4 t + i --------------------------------------------------------
  f4 d1[4];
#pragma unroll
  for (int t = 0; t < 4; t++) d1[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < SDC_ROWMLP_S2; s++) {
    const f4 a = *reinterpret_cast<const f4*>(L.actor_t.a2t[s][lane]);
#pragma unroll
    for (int t = 0; t < 4; t++) d1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], d[s >> 2][s & 3], d1[t], 0, 0, 0);
  }
  // ---- LayerNorm 1, activation 1: d1 = dZ1 --------------------------------------------------------------------------------------------
  ln_back(d1, T.l1.n, T.l1.rs, W->ln1_g, g, A.g1, A.be1);
#pragma unroll
  for (int t = 0; t < 4; t++) d1[t] = d1[t] * T.l1.dact[t];
  // ---- dW1 += dZ1 X^T (X: layer 1's input, 26 entries, then a ONE -- its column of dW1 is db1 -- and zeros to 32) -----------------------
  sdc_rowmlp::transpose_out(ta, d1, g, e);
#pragma unroll
  for (int s = 0; s < SDC_AEV_S1 - 1; s++) tb[(4 * s + g) * SDC_AGR_S + e] = x[s];
  tb[(4 * (SDC_AEV_S1 - 1) + g) * SDC_AGR_S + e] = g == 2 ? 1.0f : x[SDC_AEV_S1 - 1];      // (entry 26: the one; 27: x's zero)
  tb[(4 * SDC_AEV_S1 + g) * SDC_AGR_S + e] = 0.0f;
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
      const f2 a = *reinterpret_cast<const f2*>(L.actor_t.a1t[s][lane]);
#pragma unroll
      for (int tp = 0; tp < 2; tp++) dx[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tp], d1[s >> 2][s & 3], dx[tp], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < SDC_AEV_S1; s++) {
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
__device__ __forceinline__ void emit(float* stage, const Acc& A, const float (&w3)[SDC_AEV_OUT][4][4][4], const int lane) {
  const int g = lane >> 4, e = lane & 15;
  // register r of tile t: unit 16 t + 4 g + r
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int unit = 16 * t + 4 * g + r;
#pragma unroll
      for (int tp = 0; tp < 4; tp++) put<FIRST>(stage, SDC_AGR_W2 + unit * SDC_ROWMLP_H + 16 * tp + e, A.w2[t][tp][r]);
      put<FIRST>(stage, SDC_AGR_W1 + unit * SDC_AEV_IN + e, A.w1[t][0][r]);
    }
  if (e < SDC_AEV_IN - 16) {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) put<FIRST>(stage, SDC_AGR_W1 + (16 * t + 4 * g + r) * SDC_AEV_IN + 16 + e, A.w1[t][1][r]);
  }
  if (e == SDC_AEV_IN - 16) {      // (the column of ones)
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) put<FIRST>(stage, SDC_AGR_B1 + 16 * t + 4 * g + r, A.w1[t][1][r]);
  }
  if (e < SDC_AEV_OUT) {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) put<FIRST>(stage, SDC_AGR_W3 + e * SDC_ROWMLP_H + 16 * t + 4 * g + r, A.w3[t][r]);
  }
  if (e == 0) {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int unit = 16 * t + 4 * g + r;
        put<FIRST>(stage, SDC_AGR_LN1G + unit, A.g1[t][r]);
        put<FIRST>(stage, SDC_AGR_LN1B + unit, A.be1[t][r]);
        put<FIRST>(stage, SDC_AGR_B2 + unit, A.b2[t][r]);
        put<FIRST>(stage, SDC_AGR_LN2G + unit, A.g2[t][r]);
        // dbeta2 = W3^T db3 of this wavefront's rows
        put<FIRST>(stage, SDC_AGR_LN2B + unit, (w3[0][g][t][r] * A.b3[0] + w3[1][g][t][r] * A.b3[1]) + w3[2][g][t][r] * A.b3[2]);
      }
#pragma unroll
    for (int s = 0; s < SDC_AEV_S1; s++) {
      const int k = 4 * s + g;
      if (k < SDC_AEV_IN) {
        put<FIRST>(stage, SDC_AGR_LN0G + k, A.g0[s]);
        put<FIRST>(stage, SDC_AGR_LN0B + k, A.be0[s]);
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < SDC_AEV_OUT; c++) put<FIRST>(stage, SDC_AGR_B3 + c, A.b3[c]);
  }
}

template <int KIND>
__device__ __forceinline__ void grad_body(Lds& L, const SdcActorGrad& P) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  Acc A;
  {
    const f4 zero = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
      for (int tp = 0; tp < 4; tp++) A.w2[t][tp] = zero;
      A.w1[t][0] = A.w1[t][1] = zero;
      A.w3[t] = A.g1[t] = A.be1[t] = A.b2[t] = A.g2[t] = zero;
    }
#pragma unroll
    for (int c = 0; c < SDC_AEV_OUT; c++) A.b3[c] = 0.0f;
#pragma unroll
    for (int s = 0; s < SDC_AEV_S1; s++) A.g0[s] = A.be0[s] = 0.0f;
  }
  const long long n_pass = (P.n_rows + SDC_ACTOR_GRAD_BLOCK_ROWS - 1) / SDC_ACTOR_GRAD_BLOCK_ROWS;
  const long long stride = (long long)gridDim.x * SDC_ACTOR_GRAD_BLOCK_ROWS;
  const float dent = (float)P.dent;
  Fetched F;
  fetch(F, P, (long long)blockIdx.x * SDC_ACTOR_GRAD_BLOCK_ROWS + wave * SDC_ROWMLP_ROWS, lane);
#pragma unroll 1
  for (long long p = blockIdx.x; p < n_pass; p += gridDim.x) {
    const long long row0 = p * SDC_ACTOR_GRAD_BLOCK_ROWS + wave * SDC_ROWMLP_ROWS;
    pass<KIND>(L, A, F, P, dent, row0, row0 + stride, wave, lane);
  }

  // ---- the sixteen columns, then the four wavefronts in their order, then the workgroup's partial -----------------------------------
  col_sum(A.g1); col_sum(A.be1); col_sum(A.b2); col_sum(A.g2);
#pragma unroll
  for (int c = 0; c < SDC_AEV_OUT; c++) A.b3[c] = col_sum(A.b3[c]);
#pragma unroll
  for (int s = 0; s < SDC_AEV_S1; s++) {
    A.g0[s] = col_sum(A.g0[s]);
    A.be0[s] = col_sum(A.be0[s]);
  }
  __syncthreads();      // (the stage lies inside the tiles: every wavefront is through with them)
  if (wave == 0) emit<true>(L.u.stage, A, L.actor.w3, lane);
  __syncthreads();
#pragma unroll 1
  for (int w = 1; w < WAVES; w++) {
    if (wave == w) emit<false>(L.u.stage, A, L.actor.w3, lane);
    __syncthreads();
  }
  float* const out = P.part + (size_t)blockIdx.x * N;
  for (int j = (int)threadIdx.x; j < N; j += SDC_ACTOR_GRAD_BLOCK) out[j] = L.u.stage[j];
}

}  // namespace

// (the activation is a template parameter, as the forward's, and here a kernel each: one body's registers are all a launch pays for)
extern "C" __global__ void __launch_bounds__(SDC_ACTOR_GRAD_BLOCK, 1) sdc_actor_grad_tanh_kernel(SdcActorGrad P) {
  __shared__ Lds L;
  sdc_rowmlp::to_lds(&L.actor, P.actor);
  sdc_rowmlp::to_lds(&L.actor_t, P.actor_t);
  grad_body<0>(L, P);      // (the first pass's barrier orders the copies before the reads)
}
extern "C" __global__ void __launch_bounds__(SDC_ACTOR_GRAD_BLOCK, 1) sdc_actor_grad_relu_kernel(SdcActorGrad P) {
  __shared__ Lds L;
  sdc_rowmlp::to_lds(&L.actor, P.actor);
  sdc_rowmlp::to_lds(&L.actor_t, P.actor_t);
  grad_body<1>(L, P);
}

// a parameter's B partials in workgroup order, fp64, rounded once
extern "C" __global__ void __launch_bounds__(SDC_ACTOR_GRAD_BLOCK) sdc_actor_grad_reduce_kernel(SdcActorGradReduce P) {
  const int j = (int)(blockIdx.x * SDC_ACTOR_GRAD_BLOCK + threadIdx.x);
  if (j >= N) return;
  double s = 0.0;
  for (int b = 0; b < P.n_part; b++) s = s + (double)P.part[(size_t)b * N + j];
  P.grads[j] = (float)s;
}

// the squares of the stored fp32 gradients, fp64: lane l takes parameters l, l + 256, ... in that order, then the halving tree
extern "C" __global__ void __launch_bounds__(SDC_ACTOR_GRAD_SQ_BLOCK) sdc_actor_grad_sq_kernel(SdcActorGradSq P) {
  __shared__ double part[SDC_ACTOR_GRAD_SQ_BLOCK];
  const int l = (int)threadIdx.x;
  double s = 0.0;
  for (int j = l; j < N; j += SDC_ACTOR_GRAD_SQ_BLOCK) {
    const double v = (double)P.grads[j];
    s = s + v * v;
  }
  part[l] = s;
  __syncthreads();
  for (int half = SDC_ACTOR_GRAD_SQ_BLOCK / 2; half >= 1; half >>= 1) {
    if (l < half) part[l] = part[l] + part[l + half];
    __syncthreads();
  }
  if (l == 0) P.grad_sq[0] = part[0];
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
  const dim3 grid(sdc_actor_grad_blocks(P.n_rows)), block(SDC_ACTOR_GRAD_BLOCK);
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
