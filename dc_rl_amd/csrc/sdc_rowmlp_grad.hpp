// sdc_rowmlp_grad.hpp -- THE BACKWARD of the row network (sdc_rowmlp.hpp), once, under the actors' and the critic's gradient kernels
// (sdc_actor_grad.hip: 26 inputs, three logits; sdc_critic_grad.hip: 29 inputs, one value), and the two small kernels' bodies behind
// them: the gradient of a loss with respect to every parameter of the network over rows of stored inputs.  What differs between the
// two -- what a row brings with it, the forward's last layer, that layer's gradient and sums -- is a HEAD type of the .hip file (below).
//
// THE MAPPING IS THE FORWARD'S: a wavefront takes sixteen rows, lane l = (g = l >> 4, e = l & 15) works on row e, and the forward is
// recomputed per tile with a tape (sdc_rowmlp::Tape): 128 activations per row are cheaper to compute again than to store and fetch.
// The backward, per tile:
//   the head's gradient per row in every lane of its column: dy2, the gradient at the second hidden LayerNorm's output;
//   dY1 = W2^T dZ2 and dX = W1^T dZ1 with dZ AS IT STANDS in the accumulators as the B operand (sdc_rowmlp_grad_pack.hpp) -- no data moves;
//   dX only when the feature LayerNorm is on (nothing is propagated to the inputs);
//   dW2 += dZ2 Y1^T and dW1 += dZ1 X^T sum over ROWS: both operands need the rows on the k side, a transpose of what the lanes hold,
//   through the wavefront's own LDS tiles [unit][16 rows] (row stride SDC_ROWMLP_TS = 20 dwords: a lane's four rows are one 16-byte
//   read, the stores of a lane group fall into distinct banks; Y1^T is stored by the forward itself).  k-step q, k slot g stands for row
//   4 g + q; lane (g, e) supplies A = dZ[unit 16 t + e][rows 4 g ..] and B = Y[unit 16 t' + e][rows 4 g ..], and register r of
//   accumulator (t, t') is dW[unit 16 t + 4 g + r][input 16 t' + e]: 64 + 32 accumulation registers (and the head's) that stay in the
//   register file over every pass of the grid-stride loop.  Entry IN of X's padding is a ONE: that column of dW1 is db1.
//   The other per-unit vectors (b2, LayerNorm 1's pair, the feature LayerNorm's pair, the head's) are PER-LANE SUMS in the
//   accumulators' layout, added up across the sixteen columns once, at the end.
// gfx950's 512 registers per lane are 256 that vector instructions address and 256 accumulation registers: the tape, the per-lane sums
// and the working set fill the first, the matrix products' sums sit in the second -- ONE wavefront per SIMD, one workgroup of four per
// CU.  No lane predicate lives across the loop (the compiler keeps each as an SGPR pair): the observation tile is padded to whole
// 64-dword loads and every lane stores all its dwords, relu' is arithmetic (sdc_rowmlp.hpp).
// Per wavefront and pass: 4 S1 + 64 forward and 64 (dY1) + 64 (dW2) + 32 (dW1) + 32 (dX, feature LayerNorm on) backward MFMAs, and the head's.
//
// THE ORDER OF EVERY SUM IS FIXED, no two lanes ever add to one word at once: a lane's sums take its rows in pass order; the sixteen columns are added by a butterfly
// (xor 1, 2, 4, 8); the matrix instructions sum a tile's rows in the hardware's fixed order; the four wavefronts of a workgroup are
// added in wavefront order through LDS ((w0 + w1) + w2) + w3 into partial [workgroup][N] of the handle's buffer; `reduce` adds the B
// partials of a parameter in workgroup order in fp64 and rounds once; `grad_sq` folds (double)g * (double)g: lane l of ONE workgroup
// of 256 takes parameters l, l + 256, ... in that order, then for half = 128 .. 1 lane l < half takes lane l + half.
// B = min(ceil(n_rows / 64), the network's MAX_BLOCKS): n_rows alone.
//
// EVERY ADDRESS A LANE FORMS IS BELOW ITS ARRAY'S END.  The head's fetch loads a dword of row = row0 + r only when row < n_rows (its
// arrays' bounds: sdc_actor_grad.hpp, sdc_critic_grad.hpp);
//   part     b * N + j  < B * N, j < N; b = blockIdx < B <= MAX_BLOCKS
//   grads    j < N
// in 64-bit arithmetic.  LDS: a transposed tile's stores are (16 t + 4 g + i) * 20 + e < 1280 (X^T: (4 s + g) * 20 + e, 4 s + g <= 31:
// < 640), its 16-byte reads (16 t + e) * 20 + 4 g + 3 < 1280; the observation tile: stores lane + 64 j < 64 TILE_LOADS (448, 512), reads
// e * IN + 4 s + g <= 15 IN + 4 S1 - 1 (417, 466: the entries past IN read a neighbour's or fetch's zeros and are dropped); the stage:
// N dwords inside the tiles.  The number of passes is the same in every wavefront of a workgroup: every barrier is reached by all.  A
// row at or past n_rows computes on zeros with a zero head gradient: it adds exact zeros.
//
// A HEAD (a struct of static functions; Head in each .hip file) gives
//   IN, OUT; Dev (the forward's network in LDS), Args (the kernel's argument: n_rows and part among its members)
//   Tiles        sdc_rowmlp_grad::Tiles<IN>, or a struct derived from it with the head's own tiles behind
//   Fetched      what a lane fetches ahead for a pass: v[TILE_LOADS<IN>], its dwords of the wavefront's input tile, and `row`, a Row:
//                what row e = lane & 15 brings with it for the head's gradient
//   fetch(F, P, row0, lane)
//   Acc          the head's sums over all passes (zero-initialised by {}); Out: what its forward returns
//   forward<KIND>(W, x, lane, out, tape)
//   gradient(tiles, acc, P, row, out, tape, W, d, row0, wave, lane)           -> d = dy2, the head's per-lane sums
//   ln2_gain(acc)                                                             LayerNorm 2's gain sums, or nullptr: the head forms them
//   products(tiles, acc, wave, lane)                                          the head's own matrix product, behind dW2's barrier
//   col_sums(acc), emit<FIRST>(stage, acc, W, lane)                           its share of the end
#pragma once

#include <hip/hip_runtime.h>

#include "sdc_rowmlp.hpp"
#include "sdc_rowmlp_grad_pack.hpp"

#define SDC_ROWMLP_GRAD_SQ_BLOCK 256      // lanes of a sum-of-squares kernel (a power of two)

struct SdcRowMlpGradReduce {
  int n_part;                  // B
  const float* part;
  float* grads;                // [N]
};
struct SdcRowMlpGradSq {
  const float* grads;
  double* grad_sq;             // [1]
};

static inline int sdc_rowmlp_grad_blocks(const long long n_rows, const int max_blocks) {
  const long long want = (n_rows + SDC_ROWMLP_BLOCK_ROWS - 1) / SDC_ROWMLP_BLOCK_ROWS;
  return (int)(want < max_blocks ? want : max_blocks);
}

// where each member of a network's params struct starts in `grads`: its float members in declaration order
template <int IN, int OUT>
struct SdcRowMlpGradAt {
  static constexpr int LN0G = 0, LN0B = IN, W1 = 2 * IN, B1 = W1 + 64 * IN, LN1G = B1 + 64, LN1B = LN1G + 64, W2 = LN1B + 64,
                       B2 = W2 + 64 * 64, LN2G = B2 + 64, LN2B = LN2G + 64, W3 = LN2B + 64, B3 = W3 + OUT * 64, N = B3 + OUT;
};

namespace sdc_rowmlp_grad {

using sdc_act::f4;
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int WAVES = SDC_ROWMLP_BLOCK / 64;
constexpr int TS = SDC_ROWMLP_TS;
constexpr int TT_DW = SDC_ROWMLP_H * TS;      // a transposed tile: 64 units of 16 rows, 20 dwords apart
static_assert((SDC_ROWMLP_GRAD_SQ_BLOCK & (SDC_ROWMLP_GRAD_SQ_BLOCK - 1)) == 0, "the tree halves");

// ---- the small kernels' bodies --------------------------------------------------------------------------------------------------------
// a parameter's B partials in workgroup order, fp64, rounded once
template <int N>
__device__ __forceinline__ void reduce(const SdcRowMlpGradReduce& P) {
  const int j = (int)(blockIdx.x * SDC_ROWMLP_BLOCK + threadIdx.x);
  if (j >= N) return;
  double s = 0.0;
  for (int b = 0; b < P.n_part; b++) s = s + (double)P.part[(size_t)b * N + j];
  P.grads[j] = (float)s;
}

// the squares of the stored fp32 gradients, fp64: lane l takes parameters l, l + 256, ... in that order, then the halving tree
template <int N, int BLOCK>
__device__ __forceinline__ void grad_sq(const SdcRowMlpGradSq& P) {
  __shared__ double part[BLOCK];
  const int l = (int)threadIdx.x;
  double s = 0.0;
  for (int j = l; j < N; j += BLOCK) {
    const double v = (double)P.grads[j];
    s = s + v * v;
  }
  part[l] = s;
  __syncthreads();
  for (int half = BLOCK / 2; half >= 1; half >>= 1) {
    if (l < half) part[l] = part[l] + part[l + half];
    __syncthreads();
  }
  if (l == 0) P.grad_sq[0] = part[0];
}

// ---- the gradient kernels' LDS --------------------------------------------------------------------------------------------------------
template <int IN>
struct Tiles {
  float obs[WAVES][sdc_rowmlp::TILE_LOADS<IN> * 64];      // padded: every lane stores all its dwords, the last ones are never read
  float ta[WAVES][TT_DW];                                 // dZ^T
  float tb[WAVES][TT_DW];                                 // Y1^T (64 units), then X^T (the first 32)
};
template <class HEAD>
struct alignas(16) Lds {      // (16-byte aligned: the A operands, the per-unit vectors and the tiles are read as 16-byte units)
  typename HEAD::Dev net;
  SdcRowMlpGradDev net_t;
  union {
    typename HEAD::Tiles tile;
    float stage[SdcRowMlpGradAt<HEAD::IN, HEAD::OUT>::N];      // the workgroup's sum, once the passes are over
  } u;
  static_assert(sizeof(typename HEAD::Tiles) >= sizeof(float) * SdcRowMlpGradAt<HEAD::IN, HEAD::OUT>::N, "the stage lies inside the tiles");
  static_assert(offsetof(Tiles<HEAD::IN>, ta) % 16 == 0 && (TT_DW * sizeof(float)) % 16 == 0 && TS % 4 == 0 && sizeof(Tiles<HEAD::IN>) % 16 == 0,
                "a tile's 16-byte reads are aligned");
};

// the sums a wavefront keeps over all its passes, the head's apart
template <int S1>
struct Acc {
  f4 w2[4][4];                 // [t][t']: register r = dW2[unit 16 t + 4 g + r][unit 16 t' + e]
  f4 w1[4][2];                 // [t][t']: register r = dW1[unit 16 t + 4 g + r][entry 16 t' + e]; entry IN is a column of ones: db1
  f4 g1[4], be1[4], b2[4];     // per-lane sums in the accumulators' layout: register (t, i) = unit 16 t + 4 g + i, this column's rows
  float g0[S1], be0[S1];       // entry 4 s + g
};

// ---- helpers --------------------------------------------------------------------------------------------------------------------------
// LayerNorm(64) backward from the forward's n and rs: the gain's and the bias's sums where the caller keeps them (nullptr: it does
// not), dy -> dx = rs (dn - mean(dn) - n mean(dn n)), dn = dy gain
__device__ __forceinline__ void ln_back(f4 (&d)[4], const f4 (&n)[4], const float rs, const float (&gain)[4][4][4], const int g,
                                        f4* const dgain, f4* const dbias) {
  f4 gn[4];
  sdc_rowmlp::unit_vector(gn, gain, g);
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    if (dgain) dgain[t] = dgain[t] + d[t] * n[t];
    if (dbias) dbias[t] = dbias[t] + d[t];
  }
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

// dx -> dz = dx act'(z)
__device__ __forceinline__ void act_back(f4 (&d)[4], const f4 (&dact)[4]) {
#pragma unroll
  for (int t = 0; t < 4; t++) d[t] = d[t] * dact[t];
}

// a transposed tile (sdc_rowmlp::transpose_out stores it) back as an MFMA operand: rows 4 g .. 4 g + 3 of unit 16 t + e
__device__ __forceinline__ f4 transposed(const float* tile, const int t, const int g, const int e) {
  return *reinterpret_cast<const f4*>(tile + (16 * t + e) * TS + 4 * g);
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

// ---- the pass -------------------------------------------------------------------------------------------------------------------------
// One pass of a wavefront over rows row0 .. row0 + 15: forward with a tape, the head's gradient, the backward.  F: what was fetched for
// this pass; on return what was fetched for the next (next0; past the grid's last pass nothing is loaded).
template <int KIND, class HEAD>
__device__ __forceinline__ void pass(Lds<HEAD>& L, Acc<(HEAD::IN + 3) / 4>& A, typename HEAD::Acc& HA, typename HEAD::Fetched& F,
                                     const typename HEAD::Args& P, const long long row0, const long long next0, const int wave, const int lane) {
  constexpr int IN = HEAD::IN, S1 = (IN + 3) / 4, ONE = IN - 4 * (S1 - 1);      // the ONE: entry IN = 4 (S1 - 1) + ONE
  static_assert(IN + 1 <= 32 && ONE >= 1 && ONE <= 3, "X's tile is 32 entries, and a padded one of the last k-step is free for the ONE");
  const int g = lane >> 4, e = lane & 15;
  float* const ta = L.u.tile.ta[wave];
  float* const tb = L.u.tile.tb[wave];
  // (not the forward kernels' store and pick with their bound tests: a lane predicate costs an SGPR pair these kernels do not have --
  // the tile is padded instead, every lane stores all its dwords, the ones past 16 IN are fetch's zeros)
#pragma unroll
  for (int j = 0; j < sdc_rowmlp::TILE_LOADS<IN>; j++) L.u.tile.obs[wave][lane + 64 * j] = F.v[j];
  __syncthreads();
  // entry 4 s + g of row e; the entries from IN on (s = S1 - 1, g >= ONE) are padding: what is read there is dropped
  float x[S1];
#pragma unroll
  for (int s = 0; s < S1; s++) x[s] = L.u.tile.obs[wave][e * IN + 4 * s + g];
  x[S1 - 1] = g < ONE ? x[S1 - 1] : 0.0f;
  const typename HEAD::Row now = F.row;      // (this pass's, before the next fetch takes its place)
  HEAD::fetch(F, P, next0, lane);
  const typename HEAD::Dev* const W = &L.net;
  sdc_rowmlp::Tape<S1> T;
  T.y1t = tb;
  typename HEAD::Out out;
  HEAD::template forward<KIND>(W, x, lane, out, T);

  // ---- the head: d = dy2 ---------------------------------------------------------------------------------------------------------------
  f4 d[4];
  HEAD::gradient(L.u.tile, HA, P, now, out, T, W, d, row0, wave, lane);
  // ---- LayerNorm 2, activation 2: d = dZ2 ---------------------------------------------------------------------------------------------
  ln_back(d, T.l2.n, T.l2.rs, W->ln2_g, g, HEAD::ln2_gain(HA), nullptr);
  act_back(d, T.l2.dact);
#pragma unroll
  for (int t = 0; t < 4; t++) A.b2[t] = A.b2[t] + d[t];
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
  HEAD::products(L.u.tile, HA, wave, lane);
  // ---- dY1 = W2^T dZ2: dZ2 as it stands is the B operand of k-step s = 4 t + i --------------------------------------------------------
  f4 d1[4];
#pragma unroll
  for (int t = 0; t < 4; t++) d1[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int s = 0; s < SDC_ROWMLP_S2; s++) {
    const f4 a = *reinterpret_cast<const f4*>(L.net_t.a2t[s][lane]);
#pragma unroll
    for (int t = 0; t < 4; t++) d1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], d[s >> 2][s & 3], d1[t], 0, 0, 0);
  }
  // ---- LayerNorm 1 (its gain's and bias's sums), activation 1: d1 = dZ1 ---------------------------------------------------------------
  ln_back(d1, T.l1.n, T.l1.rs, W->ln1_g, g, A.g1, A.be1);
  act_back(d1, T.l1.dact);
  // ---- dW1 += dZ1 X^T (X: layer 1's input, IN entries, then a ONE -- its column of dW1 is db1 -- and zeros to 32) -----------------------
  sdc_rowmlp::transpose_out(ta, d1, g, e);
#pragma unroll
  for (int s = 0; s < S1 - 1; s++) tb[(4 * s + g) * TS + e] = x[s];
  tb[(4 * (S1 - 1) + g) * TS + e] = g == ONE ? 1.0f : x[S1 - 1];      // (the entries behind the ONE: x's zeros)
#pragma unroll
  for (int s = S1; s < 8; s++) tb[(4 * s + g) * TS + e] = 0.0f;
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
      const f2 a = *reinterpret_cast<const f2*>(L.net_t.a1t[s][lane]);
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

// ---- the end: a wavefront's sums into the workgroup's stage ------------------------------------------------------------------------------
template <bool FIRST, class HEAD>
__device__ __forceinline__ void emit(float* stage, const Acc<(HEAD::IN + 3) / 4>& A, const typename HEAD::Acc& HA, const typename HEAD::Dev& W,
                                     const int lane) {
  constexpr int IN = HEAD::IN, S1 = (IN + 3) / 4;
  using At = SdcRowMlpGradAt<IN, HEAD::OUT>;
  const int g = lane >> 4, e = lane & 15;
  // register r of tile t: unit 16 t + 4 g + r
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int unit = 16 * t + 4 * g + r;
#pragma unroll
      for (int tp = 0; tp < 4; tp++) put<FIRST>(stage, At::W2 + unit * SDC_ROWMLP_H + 16 * tp + e, A.w2[t][tp][r]);
      put<FIRST>(stage, At::W1 + unit * IN + e, A.w1[t][0][r]);
    }
  if (e < IN - 16) {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) put<FIRST>(stage, At::W1 + (16 * t + 4 * g + r) * IN + 16 + e, A.w1[t][1][r]);
  }
  if (e == IN - 16) {      // (the column of ones)
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) put<FIRST>(stage, At::B1 + 16 * t + 4 * g + r, A.w1[t][1][r]);
  }
  if (e == 0) {
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int unit = 16 * t + 4 * g + r;
        put<FIRST>(stage, At::LN1G + unit, A.g1[t][r]);
        put<FIRST>(stage, At::LN1B + unit, A.be1[t][r]);
        put<FIRST>(stage, At::B2 + unit, A.b2[t][r]);
      }
#pragma unroll
    for (int s = 0; s < S1; s++) {
      const int k = 4 * s + g;
      if (k < IN) {
        put<FIRST>(stage, At::LN0G + k, A.g0[s]);
        put<FIRST>(stage, At::LN0B + k, A.be0[s]);
      }
    }
  }
  HEAD::template emit<FIRST>(stage, HA, W, lane);
}

// ---- the driver: L.net and L.net_t are on their way to LDS (the first pass's barrier orders the copies before the reads) ----------------
template <int KIND, class HEAD>
__device__ __forceinline__ void grad_body(Lds<HEAD>& L, const typename HEAD::Args& P) {
  constexpr int S1 = (HEAD::IN + 3) / 4, N = SdcRowMlpGradAt<HEAD::IN, HEAD::OUT>::N;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  Acc<S1> A{};
  typename HEAD::Acc HA{};
  const long long n_pass = (P.n_rows + SDC_ROWMLP_BLOCK_ROWS - 1) / SDC_ROWMLP_BLOCK_ROWS;
  const long long stride = (long long)gridDim.x * SDC_ROWMLP_BLOCK_ROWS;
  typename HEAD::Fetched F;
  HEAD::fetch(F, P, (long long)blockIdx.x * SDC_ROWMLP_BLOCK_ROWS + wave * SDC_ROWMLP_ROWS, lane);
#pragma unroll 1
  for (long long p = blockIdx.x; p < n_pass; p += gridDim.x) {
    const long long row0 = p * SDC_ROWMLP_BLOCK_ROWS + wave * SDC_ROWMLP_ROWS;
    pass<KIND, HEAD>(L, A, HA, F, P, row0, row0 + stride, wave, lane);
  }

  // ---- the sixteen columns, then the four wavefronts in their order, then the workgroup's partial -----------------------------------
  col_sum(A.g1); col_sum(A.be1); col_sum(A.b2);
  HEAD::col_sums(HA);
#pragma unroll
  for (int s = 0; s < S1; s++) {
    A.g0[s] = col_sum(A.g0[s]);
    A.be0[s] = col_sum(A.be0[s]);
  }
  __syncthreads();      // (the stage lies inside the tiles: every wavefront is through with them)
  if (wave == 0) emit<true, HEAD>(L.u.stage, A, HA, L.net, lane);
  __syncthreads();
#pragma unroll 1
  for (int w = 1; w < WAVES; w++) {
    if (wave == w) emit<false, HEAD>(L.u.stage, A, HA, L.net, lane);
    __syncthreads();
  }
  float* const out = P.part + (size_t)blockIdx.x * N;
  for (int j = (int)threadIdx.x; j < N; j += SDC_ROWMLP_BLOCK) out[j] = L.u.stage[j];
}

}  // namespace sdc_rowmlp_grad
