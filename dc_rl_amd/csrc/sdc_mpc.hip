// sdc_mpc.hip -- sdc_mpc_start_kernel and sdc_mpc_fold_kernel: what happens between two decisions of sdc_rollout_cem_stats
// (sdc_capi.hip; the plans, the lane mapping and the address bounds: sdc_mpc.hpp; the schedule: sdc_mpc_schedule.hpp).
//
// The arithmetic is the one include/sustaindc_hip.h states for sdc_rollout_cem_stats: integer counts, and per env two fp64 additions
// and one fp64 subtraction per planned decision, no fused operation possible (the pragma below says it for this file whatever the
// flags).
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_mpc.hpp"

#pragma clang fp contract(off)

namespace {

static_assert(SDC_MPC_BLOCK % SDC_WAVE == 0, "whole wavefronts per workgroup");
static_assert(SDC_POLICY_COUNTS == 5 && SDC_POLICY_N0 == 0 && SDC_POLICY_N1 == 1 && SDC_POLICY_N2 == 2 && SDC_POLICY_SWITCHES == 3 &&
                  SDC_POLICY_LAST == 4,
              "the counts");
static_assert(SDC_PLAN_SUMS == 4 && SDC_PLAN_SCORE == 0 && SDC_PLAN_GAIN == 1 && SDC_PLAN_PLANNED == 2 && SDC_PLAN_IDLE == 3, "the sums");

typedef double f64x2 __attribute__((ext_vector_type(2)));

// a lane's 24 bytes of probs and its dword of best_seq of one step
struct Col {
  double p0, p1, p2;
  int32_t b;
};

__device__ __forceinline__ Col load_col(const double* const p, const int32_t* const b) { return Col{p[0], p[1], p[2], b[0]}; }
__device__ __forceinline__ void store_col(double* const p, int32_t* const b, const Col& c) {
  p[0] = c.p0;
  p[1] = c.p1;
  p[2] = c.p2;
  b[0] = c.b;
}

}  // namespace

// IN PLACE WITHOUT A HAZARD: the lane walks k upwards, reads step k + 1 and writes step k of ITS OWN column of probs / best_seq -- the
// 24 bytes and the dword at lane offset t of every step.  No other lane reads or writes that column, in this launch or in any launch in
// flight (the stream orders the planner's kernels around this one), and within the lane every step is read before the walk overwrites
// it: a group of SDC_MPC_UNROLL loads covers steps k + 1 .. k + U, the stores behind it steps k .. k + U - 1.
extern "C" __global__ void __launch_bounds__(SDC_MPC_BLOCK) sdc_mpc_start_kernel(SdcMpcStart P) {
  const size_t lanes = (size_t)P.n_envs * SDC_N_AGENTS;
  const size_t t = (size_t)blockIdx.x * SDC_MPC_BLOCK + threadIdx.x;
  if (t >= lanes) return;      // (no barrier below: the missing lanes of the last wavefront leave)
  const int a = (int)(t % SDC_N_AGENTS);
  const double u = 1.0 / 3.0;
  const Col start = {u, u, u, a == 0 ? P.idle[0] : (a == 1 ? P.idle[1] : P.idle[2])};
  // this lane's addresses at step 0, and what a step adds
  double* pp = P.probs + t * 3;
  int32_t* bp = P.best_seq + t;
  const size_t pstep = lanes * 3, bstep = lanes;
  const int K = P.steps;

  int k = 0;
  if (!P.fresh) {
#pragma unroll 1
    for (; k + SDC_MPC_UNROLL <= K - 1; k += SDC_MPC_UNROLL) {
      Col v[SDC_MPC_UNROLL];
#pragma unroll
      for (int i = 0; i < SDC_MPC_UNROLL; i++) v[i] = load_col(pp + (size_t)(i + 1) * pstep, bp + (size_t)(i + 1) * bstep);
#pragma unroll
      for (int i = 0; i < SDC_MPC_UNROLL; i++) store_col(pp + (size_t)i * pstep, bp + (size_t)i * bstep, v[i]);
      pp += (size_t)SDC_MPC_UNROLL * pstep;
      bp += (size_t)SDC_MPC_UNROLL * bstep;
    }
#pragma unroll 1
    for (; k < K - 1; k++) {
      const Col v = load_col(pp + pstep, bp + bstep);
      store_col(pp, bp, v);
      pp += pstep;
      bp += bstep;
    }
  }
  // the fresh fill of every step, or of the one step the shift has left: K - 1
#pragma unroll 1
  for (; k < K; k++) {
    store_col(pp, bp, start);
    pp += pstep;
    bp += bstep;
  }
}

extern "C" __global__ void __launch_bounds__(SDC_MPC_BLOCK) sdc_mpc_fold_kernel(SdcMpcFold P) {
  const size_t lanes = (size_t)P.n_envs * SDC_N_AGENTS;
  const size_t t = (size_t)blockIdx.x * SDC_MPC_BLOCK + threadIdx.x;
  if (t >= lanes) return;      // (no barrier below: the missing lanes of the last wavefront leave)
  const size_t n = t / SDC_N_AGENTS;
  const int a = (int)(t - n * SDC_N_AGENTS);
  int j;
  if (P.planned) {
    j = P.best_action[t];
  } else {
    j = a == 0 ? P.idle[0] : (a == 1 ? P.idle[1] : P.idle[2]);
    P.best_action[t] = j;
  }
  if (!P.counts) return;

  int32_t* const cnt = P.counts + t * SDC_POLICY_COUNTS;
  int n0 = 0, n1 = 0, n2 = 0, switches = 0, last = -1;
  if (!P.init) {
    n0 = cnt[SDC_POLICY_N0];
    n1 = cnt[SDC_POLICY_N1];
    n2 = cnt[SDC_POLICY_N2];
    switches = cnt[SDC_POLICY_SWITCHES];
    last = cnt[SDC_POLICY_LAST];
  }
  n0 += j == 0 ? 1 : 0;
  n1 += j == 1 ? 1 : 0;
  n2 += j == 2 ? 1 : 0;
  switches += (last >= 0 && j != last) ? 1 : 0;
  cnt[SDC_POLICY_N0] = n0;
  cnt[SDC_POLICY_N1] = n1;
  cnt[SDC_POLICY_N2] = n2;
  cnt[SDC_POLICY_SWITCHES] = switches;
  cnt[SDC_POLICY_LAST] = j;

  if (a != 0) return;
  // the env's row of sums: SCORE, GAIN | PLANNED, IDLE
  f64x2* const sums = reinterpret_cast<f64x2*>(P.sums + n * SDC_PLAN_SUMS);
  f64x2 sg = {0.0, 0.0}, pi = {0.0, 0.0};
  if (!P.init) {
    sg = sums[0];
    pi = sums[1];
  }
  if (P.planned) {
    const double s_first = P.score_first[n], s_last = P.score_last[n];
    sg.x += s_last;
    sg.y += s_last - s_first;
    pi.x += 1.0;
  } else {
    pi.y += 1.0;
  }
  sums[0] = sg;
  sums[1] = pi;
}

hipError_t sdc_mpc_start_launch(const SdcMpcStart& P, hipStream_t st) {
  const size_t lanes = (size_t)P.n_envs * SDC_N_AGENTS;
  const int blocks = (int)((lanes + SDC_MPC_BLOCK - 1) / SDC_MPC_BLOCK);
  hipLaunchKernelGGL(sdc_mpc_start_kernel, dim3(blocks), dim3(SDC_MPC_BLOCK), 0, st, P);
  return hipGetLastError();
}

hipError_t sdc_mpc_fold_launch(const SdcMpcFold& P, hipStream_t st) {
  const size_t lanes = (size_t)P.n_envs * SDC_N_AGENTS;
  const int blocks = (int)((lanes + SDC_MPC_BLOCK - 1) / SDC_MPC_BLOCK);
  hipLaunchKernelGGL(sdc_mpc_fold_kernel, dim3(blocks), dim3(SDC_MPC_BLOCK), 0, st, P);
  return hipGetLastError();
}
