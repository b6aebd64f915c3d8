// sdc_cem_groups.hip -- the cross-entropy method with the candidates in env slots (sdc_plan_cem_groups, sdc_capi.hip; the plans:
// sdc_cem_groups.hpp).  The batch is G groups of R consecutive envs that hold one state: sdc_cem_group_sample_kernel turns every
// group's per-step, per-agent categorical distribution into its R replicas' action sequences, replica 0 the incumbent;
// sdc_cem_group_refit_kernel turns the replicas' scores into the group's elite set, its new incumbent and the refitted distributions,
// and after the call's last iteration fills best_action and the broadcast step_actions.
//
// The arithmetic is the one include/sustaindc_hip.h states for sdc_plan_cem_groups, operation by operation -- sdc_plan_cem's with
// "candidate m of env n" read as "replica r of group g": fp64, no fused multiply-adds (the library is built with -ffp-contract=off),
// an IEEE division.  Every address a lane forms is below its array's end: a lane past the batch's last env loads and stores nothing,
// a group's rows are the R rows from g R on with g < G and G R = N, and the LDS arrays are sized by the constants the host refuses
// beyond (R <= SDC_CEM_MAX_GROUP; R >= 2, so 64 consecutive envs touch at most SDC_CEMG_SAMPLE_GROUPS groups -- clamped here too).
//
// SAMPLE: one wavefront per (step, 64 envs).  The 64 envs belong to groups g_lo .. g_hi, whose probabilities of the step are (g_hi -
// g_lo + 1) * 72 contiguous bytes and whose incumbent rows 12 bytes each: both are read ONCE PER GROUP, consecutive lanes on
// consecutive doubles / dwords, into LDS, where every lane picks its group's row (lanes of one group read one address: a broadcast;
// the rows of different groups lie 9 doubles / 3 dwords apart -- odd strides).  One philox4x32_10 block per lane, three thresholds,
// and the 64 envs' actions -- 768 contiguous bytes of cand[k] -- leave through LDS as consecutive lanes on consecutive dwords, not
// as 12-byte stores at a 12-byte stride.  3 552 bytes of LDS a wavefront.
//
// REFIT: one workgroup of SIXTEEN wavefronts per group (1 024 threads; with fewer, the unrolled counting below held more ballots in
// scalar registers than there are and spilled them).  The group's R scores sit in LDS (8 KiB at R = 1024).  Thread t ranks replicas
// t, t + 1024, ... -- with R <= 1024 that is replica t alone, the loop is fully unrolled -- against all R in one pass over the scores:
// every LDS read is a broadcast.  The elite set is an R-bit mask in LDS, written 64 bits at a time from wavefront ballots (replicas
// 64 j .. 64 j + 63 are one wavefront's lanes); the lowest-numbered replica of rank 0 comes from an LDS atomicMin (one replica,
// unless scores are NaN).  Per step, the group's cand rows are 12 R contiguous bytes: thread t holds dwords t, t + 1024, t + 2048 of
// them (one unrolled run of consecutive lanes on consecutive dwords); dword u is agent u % 3 of replica u / 3, whose elite bit and
// "is the best" bit the thread looked up once, before the step loop.  The nine elite counts of a step are population counts of
// wavefront ballots -- three ballots per 64 dwords: the elites' lanes and the two bits of the action; the agents' lanes are constant
// masks --, kept in scalar registers, handed over through LDS [2][16][9] -- double buffered, so a step costs ONE barrier -- and
// summed by the three lanes (one per agent) that refit the step's probabilities; no per-lane atomics.  The lanes that hold the best
// replica's dwords write them to best_seq; replica 0 is the incumbent (the sample kernel put it there), so best = 0 rewrites an
// unbeaten incumbent with its own bits.  After the last iteration the step-0 row goes through LDS to every thread, which fills the
// group's 12 R contiguous bytes of step_actions, and to best_action.  A wavefront past the group's last replica / dword only keeps
// the barriers.
// Nothing is indexed dynamically in registers (every loop over a register array is fully unrolled), so nothing goes to scratch.
#include <hip/hip_runtime.h>

#include "sdc_cem.hpp"
#include "sdc_cem_groups.hpp"
#include "sdc_device.hpp"

namespace {

constexpr int ROW_P = SDC_N_AGENTS * 3;      // doubles per group and step in probs
constexpr int ROW_A = SDC_N_AGENTS;          // dwords per env (group) and step in cand (best_seq)
constexpr int T = SDC_CEMG_REFIT_BLOCK;
static_assert(SDC_N_AGENTS == 3, "words x, y, z of one philox block serve the three agents");
static_assert(SDC_CEMG_SAMPLE_BLOCK == SDC_WAVE, "one lane per env, 64-lane wavefronts");
static_assert(SDC_CEMG_SAMPLE_GROUPS == (SDC_CEMG_SAMPLE_BLOCK - 1) / 2 + 2, "groups of two or more envs that 64 consecutive envs can touch");
static_assert(SDC_CEM_MAX_GROUP % T == 0 && SDC_CEM_MAX_GROUP % SDC_WAVE == 0, "whole wavefronts of replicas, whole mask words");
static_assert(SDC_CEMG_RANK_PER_THREAD * T == SDC_CEM_MAX_GROUP && SDC_CEMG_ROW_PER_THREAD * T == ROW_A * SDC_CEM_MAX_GROUP,
              "the threads' register arrays cover a group of the largest size");
// the lanes whose number is 0, 1, 2 modulo 3
constexpr unsigned long long LANES_0 = 0x9249249249249249ull, LANES_1 = 0x2492492492492492ull, LANES_2 = 0x4924924924924924ull;
static_assert((LANES_0 ^ LANES_1 ^ LANES_2) == ~0ull && (LANES_0 & 1ull) && (LANES_1 & 2ull) && (LANES_2 & 4ull), "a partition of the 64 lanes");
static_assert(SDC_CEMG_ROW_PER_THREAD <= 32, "the elite and best bits of a thread's dwords are one register each");

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_CEMG_SAMPLE_BLOCK) sdc_cem_group_sample_kernel(SdcCemGroupSample P) {
  __shared__ double s_p[SDC_CEMG_SAMPLE_GROUPS * ROW_P];
  __shared__ int32_t s_b[SDC_CEMG_SAMPLE_GROUPS * ROW_A];
  __shared__ int32_t s_a[SDC_CEMG_SAMPLE_BLOCK * ROW_A];
  const int lane = (int)threadIdx.x, N = P.n_envs, R = P.group_size, G = P.n_groups, K = P.n_steps, k = (int)blockIdx.y;
  const int env0 = (int)blockIdx.x * SDC_CEMG_SAMPLE_BLOCK, env = env0 + lane;
  const int rows = min(N - env0, SDC_CEMG_SAMPLE_BLOCK);
  const bool live = lane < rows;
  // the groups of this wavefront's envs: their probabilities and incumbent rows of step k, once per group
  const int g_lo = env0 / R;
  const int n_g = min(min((env0 + rows - 1) / R, G - 1) - g_lo + 1, SDC_CEMG_SAMPLE_GROUPS);
  const size_t grp0 = (size_t)k * (size_t)G + (size_t)g_lo;
  for (int u = lane; u < n_g * ROW_P; u += SDC_WAVE) s_p[u] = P.probs[grp0 * ROW_P + u];
  for (int u = lane; u < n_g * ROW_A; u += SDC_WAVE) s_b[u] = P.best_seq[grp0 * ROW_A + u];
  __syncthreads();
  if (live) {
    const int g = env / R, r = env - g * R;
    const int gl = min(g - g_lo, n_g - 1);
    const Philox4 x = philox4x32_10((unsigned)(r * K + k), (unsigned)(P.group_base + g), P.draw, P.c3, P.key0, P.key1);
    const unsigned word[SDC_N_AGENTS] = {x.x, x.y, x.z};
#pragma unroll
    for (int a = 0; a < SDC_N_AGENTS; a++) {
      const double lo = s_p[gl * ROW_P + a * 3];      // p0, and p0 + p1 (p2 is never read)
      const double hi = lo + s_p[gl * ROW_P + a * 3 + 1];
      const double u = (double)word[a] * (1.0 / 4294967296.0);
      const int act = (int)(u >= lo) + (int)(u >= hi);
      // replica 0: the incumbent
      s_a[lane * ROW_A + a] = r == 0 ? s_b[gl * ROW_A + a] : P.fixed[a] >= 0 ? P.fixed[a] : act;
    }
  }
  __syncthreads();
  // the 64 envs' rows of cand[k]: consecutive lanes on consecutive dwords
  int32_t* const dst = P.cand + ((size_t)k * (size_t)N + (size_t)env0) * ROW_A;
#pragma unroll
  for (int i = 0; i < ROW_A; i++) {
    const int u = lane + SDC_WAVE * i;
    if (u < rows * ROW_A) dst[u] = s_a[u];
  }
}

extern "C" __global__ void __launch_bounds__(SDC_CEMG_REFIT_BLOCK) sdc_cem_group_refit_kernel(SdcCemGroupRefit P) {
  __shared__ double s_score[SDC_CEM_MAX_GROUP];
  __shared__ unsigned long long s_mask[SDC_CEM_MAX_GROUP / SDC_WAVE];
  __shared__ unsigned s_cnt[2][SDC_CEMG_REFIT_WAVES][ROW_P];
  __shared__ int32_t s_act[ROW_A];
  __shared__ int s_best;
  const int t = (int)threadIdx.x, lane = t & (SDC_WAVE - 1);
  const int w = __builtin_amdgcn_readfirstlane(t / SDC_WAVE);      // (the same in every lane: in a scalar register)
  const int N = P.n_envs, R = min(P.group_size, SDC_CEM_MAX_GROUP), G = P.n_groups, K = P.n_steps, g = (int)blockIdx.x;
  const size_t env0 = (size_t)g * (size_t)R;      // g < G and G R = N: the group's rows are env0 .. env0 + R - 1 < N
  for (int c = t; c < R; c += T) s_score[c] = P.score[env0 + (size_t)c];
  if (t == 0) s_best = R;
  __syncthreads();
  // rank(c) = the replicas that score higher, or the same with a lower number; elite: rank < E; the incumbent-to-be: rank 0
  {
    double s[SDC_CEMG_RANK_PER_THREAD];
    int rank[SDC_CEMG_RANK_PER_THREAD];
#pragma unroll
    for (int i = 0; i < SDC_CEMG_RANK_PER_THREAD; i++) {
      const int c = t + i * T;
      s[i] = c < R ? s_score[c] : 0.0;
      rank[i] = 0;
    }
    if (w * SDC_WAVE < R) {      // (a wavefront past the group's last replica ranks nothing)
#pragma unroll 2
      for (int o = 0; o < R; o++) {
        const double x = s_score[o];
#pragma unroll
        for (int i = 0; i < SDC_CEMG_RANK_PER_THREAD; i++) rank[i] += (int)((x > s[i]) | ((x == s[i]) & (o < t + i * T)));
      }
    }
#pragma unroll
    for (int i = 0; i < SDC_CEMG_RANK_PER_THREAD; i++) {
      const int c = t + i * T;      // replicas 64 (w + 16 i) .. + 63 are this wavefront's lanes
      const bool in = c < R;
      const unsigned long long elite = __ballot(in && rank[i] < P.n_elite);
      if (lane == 0) s_mask[w + i * SDC_CEMG_REFIT_WAVES] = elite;
      if (in && rank[i] == 0) atomicMin(&s_best, c);      // (one replica, unless scores are NaN: then the lowest-numbered of them)
    }
  }
  __syncthreads();
  const int best = min(s_best, R - 1);
  if (t == 0) P.best_score[g] = s_score[best];
  // dword u = t + 1024 i of a step's rows is agent u % 3 of replica u / 3: that replica's elite bit, and whether it is the best
  unsigned ebits = 0u, bbits = 0u;
#pragma unroll
  for (int i = 0; i < SDC_CEMG_ROW_PER_THREAD; i++) {
    const int rep = (t + i * T) / ROW_A;
    if (rep < R) {
      ebits |= (unsigned)((s_mask[rep / SDC_WAVE] >> (rep & (SDC_WAVE - 1))) & 1ull) << i;
      bbits |= (unsigned)(rep == best) << i;
    }
  }
  const int agent = t < ROW_A ? t : 0;      // lanes 0..2 refit one agent's probabilities each
  const int fixed_a = agent == 0 ? P.fixed[0] : agent == 1 ? P.fixed[1] : P.fixed[2];
  const bool refits = t < ROW_A && fixed_a < 0;      // an agent with a fixed action keeps its probabilities
  const double n_e = (double)P.n_elite;
#pragma unroll 1
  for (int k = 0; k < K; k++) {
    const int32_t* const row = P.cand + ((size_t)k * (size_t)N + env0) * ROW_A;
    const size_t grp = (size_t)k * (size_t)G + (size_t)g;
    int32_t v[SDC_CEMG_ROW_PER_THREAD];
#pragma unroll
    for (int i = 0; i < SDC_CEMG_ROW_PER_THREAD; i++) {
      const int u = t + i * T;
      v[i] = u < R * ROW_A ? row[u] : 0;
    }
    double* const p = P.probs + grp * ROW_P + agent * 3;
    double p_old[3] = {0.0, 0.0, 0.0};
    if (refits) {
#pragma unroll
      for (int j = 0; j < 3; j++) p_old[j] = p[j];
    }
    unsigned cnt[ROW_P] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};      // [agent][action]: this wavefront's elites
#pragma unroll
    for (int i = 0; i < SDC_CEMG_ROW_PER_THREAD; i++) {
      if (i * T + w * SDC_WAVE < R * ROW_A) {      // (the same in every lane)
        const int u = t + i * T, am = u % ROW_A;
        // three ballots: the elites' lanes and the two bits of the action; whose agent a lane's dword is follows from the lane
        // number alone (lane 0 holds agent (64 w + T i) % 3), so the agents' lanes are three constant masks
        const unsigned long long el = __ballot(((ebits >> i) & 1u) != 0u);
        const unsigned long long b0 = __ballot((v[i] & 1) != 0), b1 = __ballot((v[i] & 2) != 0);
        const unsigned long long act[3] = {~b0 & ~b1, b0 & ~b1, ~b0 & b1};
        const int first = (w * SDC_WAVE + i * T) % ROW_A;
#pragma unroll
        for (int a = 0; a < SDC_N_AGENTS; a++) {
          const int c = (a - first + ROW_A) % ROW_A;      // agent a: the lanes with lane % 3 == c
          const unsigned long long mine = el & (c == 0 ? LANES_0 : c == 1 ? LANES_1 : LANES_2);
#pragma unroll
          for (int j = 0; j < 3; j++) cnt[a * 3 + j] += (unsigned)__popcll(mine & act[j]);
        }
        if ((bbits >> i) & 1u) {      // the new incumbent's step (best = 0: the bits it had)
          P.best_seq[grp * ROW_A + am] = v[i];
          if (k == 0) s_act[am] = v[i];
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < ROW_P; q++) s_cnt[k & 1][w][q] = cnt[q];
    }
    __syncthreads();      // (the one barrier of a step: the next step fills the other half of s_cnt)
    if (refits) {
      double q[3];
#pragma unroll
      for (int j = 0; j < 3; j++) {
        unsigned c = 0u;
#pragma unroll
        for (int ww = 0; ww < SDC_CEMG_REFIT_WAVES; ww++) c += s_cnt[k & 1][ww][agent * 3 + j];
        const double tj = (double)c / n_e;
        const double x = P.alpha * p_old[j] + P.take * tj;
        q[j] = x < P.p_min ? P.p_min : x;
      }
      const double s = (q[0] + q[1]) + q[2];
#pragma unroll
      for (int j = 0; j < 3; j++) p[j] = q[j] / s;
    }
    if (k == 0 && P.last) {      // best_action = best_seq[0], and every replica's row of step_actions
      if (t < ROW_A) P.best_action[(size_t)g * ROW_A + t] = s_act[t];
      int32_t* const out = P.step_actions + env0 * ROW_A;
#pragma unroll
      for (int i = 0; i < SDC_CEMG_ROW_PER_THREAD; i++) {
        const int u = t + i * T;
        if (u < R * ROW_A) out[u] = s_act[u % ROW_A];
      }
    }
  }
}

hipError_t sdc_cem_group_sample_launch(const SdcCemGroupSample& P, hipStream_t st) {
  const int blocks = (P.n_envs + SDC_CEMG_SAMPLE_BLOCK - 1) / SDC_CEMG_SAMPLE_BLOCK;
  hipLaunchKernelGGL(sdc_cem_group_sample_kernel, dim3(blocks, P.n_steps), dim3(SDC_CEMG_SAMPLE_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_cem_group_refit_launch(const SdcCemGroupRefit& P, hipStream_t st) {
  hipLaunchKernelGGL(sdc_cem_group_refit_kernel, dim3(P.n_groups), dim3(SDC_CEMG_REFIT_BLOCK), 0, st, P);
  return hipGetLastError();
}
