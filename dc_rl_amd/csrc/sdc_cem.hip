// sdc_cem.hip -- sdc_cem_sample_kernel: every env's per-step, per-agent categorical distribution -> the iteration's candidate action
// sequences, candidate 0 the incumbent; sdc_cem_refit_kernel: the candidates' scores -> every env's elite set, its new incumbent and
// the distributions refitted to the elites (sdc_plan_cem, sdc_capi.hip; the plans: sdc_cem.hpp).
//
// The arithmetic is the one include/sustaindc_hip.h states for sdc_plan_cem, operation by operation: fp64, no fused multiply-adds (the
// library is built with -ffp-contract=off), an IEEE division.  Every address a lane forms is below its array's end: a lane past the
// batch's last env loads and stores nothing, and the last workgroup's row copies stop at the batch's last row.
//
// HOW THE ROWS MOVE.  For a fixed (candidate, step) the actions of 64 consecutive envs are 768 contiguous bytes, and for a fixed step
// their probabilities 4 608 (72 per env).  A lane that moved its own env's row would issue 12-byte stores (8-byte loads) at a 12-byte
// (72-byte) stride; instead every run goes through LDS and moves as consecutive lanes on consecutive dwords (actions) or doubles
// (probabilities): each wavefront instruction is one contiguous run of 256 or 512 bytes.  Not 16-byte units: a run starts at
// (step * N + env0) rows, which for an odd N is 4-byte (8-byte) aligned and no more.  In LDS a lane picks its row at a stride of 3
// dwords / 9 doubles -- odd, so the lanes of a group fall on distinct banks.
//
// SAMPLE: one wavefront per (step, 64 envs); it reads the step's probabilities once, copies the incumbent's row into candidate 0 and
// loops over candidates 1 .. M-1: one philox4x32_10 block per lane, three thresholds, the 192 actions out through LDS.  5 376 bytes of
// LDS a wavefront: 30 wavefronts fit a CU's 160 KiB, the register file's limit is reached first.
//
// REFIT: 64 envs per workgroup of FOUR wavefronts.  The workgroup's scores [M][64] sit in LDS (32 KiB at M = 64), and a workgroup of
// one wavefront would then leave five wavefronts per CU; with four wavefronts sharing the tile -- wavefront w ranks candidates w,
// w + 4, ... against all M, then refits steps w, w + 4, ... -- the 37 KiB a workgroup holds leave four workgroups, 16 wavefronts, per
// CU: four per SIMD.  The elite set is a 64-bit mask in a register pair (M <= 64) and the per-action elite counts are 8-bit fields
// of one register per agent (a count is at most 64), so nothing is indexed dynamically and nothing goes to scratch memory.  Once
// the ranks are known the score tile is dead, and each wavefront stages its step's probabilities in its own 4 608 bytes of it.  The
// counts read cand[m][k][n][:] for a uniform (m, k): 768 contiguous bytes per wavefront, as the score kernel reads its rewards.  These
// reads are the one row move that does NOT take the LDS route above: each lane loads its own env's three dwords (one 12-byte load at a
// 12-byte stride), M times per step -- the wavefront's load still covers exactly those 768 bytes, and staging M rows per step
// through LDS would cost M more barriers per step for it.
// Candidate 0 is the incumbent (the sample kernel put it there), so the new incumbent's step is whatever candidate `best` holds, best
// = 0 included: the row is captured in the counting loop and written back for every env, which leaves an unbeaten incumbent's bits as
// they were.
#include <hip/hip_runtime.h>

#include "sdc_cem.hpp"
#include "sdc_device.hpp"

namespace {

constexpr int ROW_P = SDC_N_AGENTS * 3;      // doubles per env and step in probs
constexpr int ROW_A = SDC_N_AGENTS;          // dwords per env and step in cand / best_seq
constexpr int TILE = SDC_CEM_REFIT_ENVS * SDC_CEM_MAX_CAND;      // doubles in the refit kernel's score tile
static_assert(SDC_N_AGENTS == 3, "words x, y, z of one philox block serve the three agents");
static_assert(SDC_CEM_SAMPLE_BLOCK == SDC_WAVE && SDC_CEM_REFIT_ENVS == SDC_WAVE, "one lane per env, 64-lane wavefronts");
static_assert(SDC_CEM_MAX_CAND <= 64, "the elite set is a 64-bit mask, an elite count an 8-bit field");
static_assert(SDC_CEM_REFIT_WAVES * SDC_CEM_REFIT_ENVS * ROW_P <= TILE, "the wavefronts' probability rows fit the dead score tile");
static_assert(4 * (TILE * 8 + SDC_CEM_REFIT_WAVES * SDC_CEM_REFIT_ENVS * (8 + 4 * ROW_A) + SDC_CEM_REFIT_ENVS * 4) <= 160 * 1024,
              "four refit workgroups -- 16 wavefronts, four per SIMD -- fit a CU's LDS");

// rows x width consecutive elements between global memory and LDS, consecutive lanes on consecutive elements
template <int WIDTH, typename T>
__device__ __forceinline__ void run_in(T* lds, const T* src, const int lane, const int rows) {
#pragma unroll
  for (int i = 0; i < WIDTH; i++) {
    const int u = lane + SDC_WAVE * i;
    if (u < rows * WIDTH) lds[u] = src[u];
  }
}
template <int WIDTH, typename T>
__device__ __forceinline__ void run_out(T* dst, const T* lds, const int lane, const int rows) {
#pragma unroll
  for (int i = 0; i < WIDTH; i++) {
    const int u = lane + SDC_WAVE * i;
    if (u < rows * WIDTH) dst[u] = lds[u];
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_CEM_SAMPLE_BLOCK) sdc_cem_sample_kernel(SdcCemSample P) {
  __shared__ double s_p[SDC_CEM_SAMPLE_BLOCK * ROW_P];
  __shared__ int32_t s_a[SDC_CEM_SAMPLE_BLOCK * ROW_A];
  const int lane = (int)threadIdx.x, N = P.n_envs, K = P.n_steps, k = (int)blockIdx.y;
  const int env0 = (int)blockIdx.x * SDC_CEM_SAMPLE_BLOCK, env = env0 + lane;
  const int rows = min(N - env0, SDC_CEM_SAMPLE_BLOCK);
  const bool live = lane < rows;
  const size_t row0 = (size_t)k * (size_t)N + (size_t)env0;      // the run's first row within a candidate
  run_in<ROW_P>(s_p, P.probs + row0 * ROW_P, lane, rows);
  // candidate 0: the incumbent
  run_in<ROW_A>(s_a, P.best_seq + row0 * ROW_A, lane, rows);
  __syncthreads();
  run_out<ROW_A>(P.cand + row0 * ROW_A, s_a, lane, rows);
  // p0 and p0 + p1 of the three agents (p2 is never read)
  double lo[SDC_N_AGENTS], hi[SDC_N_AGENTS];
#pragma unroll
  for (int a = 0; a < SDC_N_AGENTS; a++) {
    lo[a] = live ? s_p[lane * ROW_P + a * 3] : 0.0;
    hi[a] = lo[a] + (live ? s_p[lane * ROW_P + a * 3 + 1] : 0.0);
  }
  __syncthreads();
#pragma unroll 1
  for (int m = 1; m < P.n_cand; m++) {
    const Philox4 r = philox4x32_10((unsigned)(m * K + k), (unsigned)(P.env_base + env), P.draw, P.c3, P.key0, P.key1);
    const unsigned word[SDC_N_AGENTS] = {r.x, r.y, r.z};
#pragma unroll
    for (int a = 0; a < SDC_N_AGENTS; a++) {
      const double u = (double)word[a] * (1.0 / 4294967296.0);
      const int act = (int)(u >= lo[a]) + (int)(u >= hi[a]);
      s_a[lane * ROW_A + a] = P.fixed[a] >= 0 ? P.fixed[a] : act;
    }
    __syncthreads();
    run_out<ROW_A>(P.cand + (((size_t)m * (size_t)K) * (size_t)N + row0) * ROW_A, s_a, lane, rows);
    __syncthreads();
  }
}

extern "C" __global__ void __launch_bounds__(SDC_CEM_REFIT_ENVS * SDC_CEM_REFIT_WAVES) sdc_cem_refit_kernel(SdcCemRefit P) {
  __shared__ double s_tile[TILE];      // the scores [M][64]; after the ranking: the wavefronts' probability rows [4][64 * 9]
  __shared__ unsigned long long s_mask[SDC_CEM_REFIT_WAVES][SDC_CEM_REFIT_ENVS];
  __shared__ int32_t s_act[SDC_CEM_REFIT_WAVES][SDC_CEM_REFIT_ENVS * ROW_A];
  __shared__ int s_best[SDC_CEM_REFIT_ENVS];
  const int lane = (int)threadIdx.x & (SDC_WAVE - 1), w = (int)threadIdx.x / SDC_WAVE;
  const int N = P.n_envs, M = P.n_cand, K = P.n_steps;
  const int env0 = (int)blockIdx.x * SDC_CEM_REFIT_ENVS, env = env0 + lane;
  const int rows = min(N - env0, SDC_CEM_REFIT_ENVS);
  const bool live = lane < rows;
  if (live)
    for (int c = w; c < M; c += SDC_CEM_REFIT_WAVES) s_tile[c * SDC_CEM_REFIT_ENVS + lane] = P.score[(size_t)c * (size_t)N + (size_t)env];
  if (w == 0) s_best[lane] = M;
  __syncthreads();
  // rank(c) = the candidates that score higher, or the same with a lower number; elite: rank < E; the incumbent-to-be: rank 0
  unsigned long long mask = 0ull;
  if (live) {
#pragma unroll 1
    for (int c = w; c < M; c += SDC_CEM_REFIT_WAVES) {
      const double s = s_tile[c * SDC_CEM_REFIT_ENVS + lane];
      int rank = 0;
#pragma unroll 4
      for (int o = 0; o < M; o++) {
        const double x = s_tile[o * SDC_CEM_REFIT_ENVS + lane];
        rank += (int)((x > s) | ((x == s) & (o < c)));
      }
      if (rank < P.n_elite) mask |= 1ull << c;
      if (rank == 0) atomicMin(&s_best[lane], c);      // (one candidate, unless scores are NaN: then the lowest-numbered of them)
    }
  }
  s_mask[w][lane] = mask;
  __syncthreads();
  int best = 0;
  double top = 0.0;
  if (live) {
    mask = (s_mask[0][lane] | s_mask[1][lane]) | (s_mask[2][lane] | s_mask[3][lane]);
    best = s_best[lane];
    top = s_tile[best * SDC_CEM_REFIT_ENVS + lane];
  }
  static_assert(SDC_CEM_REFIT_WAVES == 4, "the four partial masks");
  __syncthreads();      // the score tile is dead from here
  if (w == 0 && live) P.best_score[env] = top;
  double* const my_p = s_tile + w * (SDC_CEM_REFIT_ENVS * ROW_P);
  int32_t* const my_a = s_act[w];
  const double n_e = (double)P.n_elite;
#pragma unroll 1
  for (int k0 = 0; k0 < K; k0 += SDC_CEM_REFIT_WAVES) {      // (every wavefront takes every trip: the barriers are the workgroup's)
    const int k = k0 + w;
    const bool has = k < K;
    const size_t row0 = (size_t)(has ? k : 0) * (size_t)N + (size_t)env0;
    if (has) run_in<ROW_P>(my_p, P.probs + row0 * ROW_P, lane, rows);
    unsigned cnt[SDC_N_AGENTS] = {0u, 0u, 0u};      // per agent: the elites' count of action j in bits 8 j .. 8 j + 7
    if (has && live) {
      int32_t keep[SDC_N_AGENTS] = {0, 0, 0};
#pragma unroll 2
      for (int m = 0; m < M; m++) {
        const int32_t* const a = P.cand + (((size_t)m * (size_t)K) * (size_t)N + row0 + (size_t)lane) * ROW_A;
        const int32_t a0 = a[0], a1 = a[1], a2 = a[2];
        const unsigned e = (unsigned)(mask >> m) & 1u;
        cnt[0] += e << (8 * (a0 & 3));
        cnt[1] += e << (8 * (a1 & 3));
        cnt[2] += e << (8 * (a2 & 3));
        if (m == best) {
          keep[0] = a0;
          keep[1] = a1;
          keep[2] = a2;
        }
      }
#pragma unroll
      for (int a = 0; a < SDC_N_AGENTS; a++) my_a[lane * ROW_A + a] = keep[a];
    }
    __syncthreads();
    if (has && live) {
#pragma unroll
      for (int a = 0; a < SDC_N_AGENTS; a++) {
        if (P.fixed[a] >= 0) continue;      // (the same in every lane) a fixed agent's probabilities stay as they are
        double* const p = my_p + lane * ROW_P + a * 3;
        double q[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const double t = (double)((cnt[a] >> (8 * j)) & 0xFFu) / n_e;
          const double x = P.alpha * p[j] + P.take * t;
          q[j] = x < P.p_min ? P.p_min : x;
        }
        const double s = (q[0] + q[1]) + q[2];
#pragma unroll
        for (int j = 0; j < 3; j++) p[j] = q[j] / s;
      }
    }
    __syncthreads();
    if (has) {
      run_out<ROW_P>(P.probs + row0 * ROW_P, my_p, lane, rows);
      run_out<ROW_A>(P.best_seq + row0 * ROW_A, my_a, lane, rows);
      if (k == 0 && P.last) run_out<ROW_A>(P.best_action + (size_t)env0 * ROW_A, my_a, lane, rows);
    }
    __syncthreads();
  }
}

hipError_t sdc_cem_sample_launch(const SdcCemSample& P, hipStream_t st) {
  const int blocks = (P.n_envs + SDC_CEM_SAMPLE_BLOCK - 1) / SDC_CEM_SAMPLE_BLOCK;
  hipLaunchKernelGGL(sdc_cem_sample_kernel, dim3(blocks, P.n_steps), dim3(SDC_CEM_SAMPLE_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_cem_refit_launch(const SdcCemRefit& P, hipStream_t st) {
  const int blocks = (P.n_envs + SDC_CEM_REFIT_ENVS - 1) / SDC_CEM_REFIT_ENVS;
  hipLaunchKernelGGL(sdc_cem_refit_kernel, dim3(blocks), dim3(SDC_CEM_REFIT_ENVS * SDC_CEM_REFIT_WAVES), 0, st, P);
  return hipGetLastError();
}
