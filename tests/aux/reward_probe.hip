// reward_probe.hip -- TEST INFRASTRUCTURE: the history-normalised reward's device code (dc_rl_amd/csrc/sdc_trackers.hpp, sdc_halfwin.hpp,
// sdc_quadwin.hpp, sdc_ringpath.hpp; the half-wave fp64 sum of sdc_pairstep.hpp), one function per kernel, so that
// tests/test_gpu_reward_functions.py can hold each function to the sorted-list model of tests/reward_model.py on the inputs of
// tests/reward_cases.py.  This file includes the product's headers themselves and restates none of their expressions; what it adds is
// the plumbing the step kernels have around them (operands from memory, results to memory, n tracked from step to step as the step does).
//
// One case is one workgroup (keys / bounds / moments: one element per thread).  One wavefront per workgroup, except refill_coop: the four
// wavefronts of a sweep workgroup (sdc_sweep.hpp serve_recentring_requests_coop).  window_ops carries 1 / 2 / 4 slots per wavefront for
// QTrack / HWin / QWin -- one per env of the mapping.  Every launcher takes device pointers, a case count and a stream and returns the
// hipError_t of the launch.  Buffer layouts stand at each kernel; tests/reward_probe.py mirrors them.
//
// NOT HERE: the lane-per-env window code, which sits inside the kernel body of sdc_wide.hip and cannot be called without moving product
// code.  It stays held by the every-env equality tests against the quad kernel (tests/test_gpu_wide.py).
//
// Inputs must keep every index the functions form in range: 0 <= hi <= 64 (refill: 1 <= hi), 2 <= n <= SDC_HIST_STRIDE, patch_slot in
// -1 .. SDC_HIST_STRIDE - 1, rings of exactly SDC_HIST_STRIDE keys with KEY_NONE in empty slots, bisect_build ranks in 0 .. n - 1 with at
// most 64 ranks per window.  tests/reward_cases.py asserts these before anything is launched.
// Built by tests/reward_probe.py with the library's compiler flags; nothing in dc_rl_amd/ knows about it.
#include "../../dc_rl_amd/csrc/sdc_pairstep.hpp"

namespace {
using namespace sdc_rw;
using sdc_hw::HWin;
using sdc_hw::QWin;

// ---- keys: in bits[n]; out [2][n]: f32_key(bits), bits of key_f32(f32_key(bits)) -------------------------------------------------------------
__global__ __launch_bounds__(256) void keys_kernel(const unsigned* __restrict__ in, unsigned* __restrict__ out, const int n) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  const unsigned k = f32_key(__uint_as_float(in[i]));
  out[i] = k;
  out[(size_t)n + i] = __float_as_uint(key_f32(k));
}

// ---- reduce: in u[case][64], d[case][64]; out ou[case][5][64] = wave sum / min / max, half sum, row sum; od[case][3][64] = wave, half, row sum
__global__ __launch_bounds__(64) void reduce_kernel(const unsigned* __restrict__ u, const double* __restrict__ d, unsigned* __restrict__ ou,
                                                    double* __restrict__ od) {
  const int lane = (int)threadIdx.x;
  const size_t c = blockIdx.x;
  const unsigned x = u[c * 64 + lane];
  const double v = d[c * 64 + lane];
  unsigned* o = ou + c * 5 * 64 + lane;
  o[0] = wave_sum_u32(x);
  o[64] = wave_min_u32(x);
  o[128] = wave_max_u32(x);
  o[192] = sdc_hw::half_sum_u32(x);
  o[256] = sdc_hw::row_sum_u32(x);
  double* p = od + c * 3 * 64 + lane;
  p[0] = wave_sum_f64(v);
  p[64] = half_sum_f64(v);
  p[128] = sdc_hw::row_sum_f64(v);
}

// ---- window_ops ------------------------------------------------------------------------------------------------------------------------------
// in  keys0[S][64], meta[S][4] = r0, hi, n0, on; ops[S][T][4] = x_new, x_old, has_old, -; iv[S][T][4] = lo0, hi0, lo1, hi1 (interval 0 with
//     flip 0, interval 1 with flip KEY_NONE: the upper and the lower clip bound's windows)
// out okeys[S][T][64]; oi[S][T][OI]; od[S][T][4] = s1, s2 of interval 0, s1, s2 of interval 1
enum { OI_R0 = 0, OI_HI, OI_CH, OI_OK1, OI_A1, OI_B1, OI_OK3, OI_A3, OI_B3, OI_SPAN0, OI_SPAN1, OI_ANY0, OI_C0, OI_ANY1, OI_C1, OI_FIRST,
       OI_LAST, OI_N, OI = 20 };
constexpr unsigned NOT_APPLICABLE = 2u;
struct OpsArgs {
  const unsigned* keys0;
  const int* meta;
  const unsigned* ops;
  const unsigned* iv;
  unsigned* okeys;
  unsigned* oi;
  double* od;
  int S, T;
};
struct Crossed {
  bool any;
  unsigned c;
  double s1, s2;
};

struct FormQTrack {   // one env per wavefront; `on` does not exist in this form
  using Win = QTrack;
  static constexpr int LPE = 64, KPL = 1;
  static constexpr bool HAS_ON = false;
  __device__ static Win make(const unsigned (&k)[1], int r0, int hi) { return QTrack{k[0], r0, hi}; }
  __device__ static void keys(const Win& q, unsigned (&k)[1]) { k[0] = q.w; }
  __device__ static bool update(Win& q, unsigned xn, unsigned xo, bool has_old, int n_prev, bool, int, int l) {
    return qt_update(q, xn, xo, has_old, n_prev, l);
  }
  __device__ static bool resolve(const Win& q, int k, int n, int, unsigned& a, unsigned& b) { return qt_resolve(q, k, n, a, b); }
  __device__ static unsigned spans(const Win& q, unsigned lo, unsigned hi, int n, int) { return qt_spans(q, lo, hi, n) ? 1u : 0u; }
  __device__ static unsigned first(const Win& q, int) { return lane_key(q.w, 0); }
  __device__ static unsigned last(const Win& q, int) { return lane_key(q.w, max(q.hi - 1, 0)); }
  __device__ static Crossed crossed(const Win& q, unsigned lo, unsigned hi, unsigned flip, bool) {   // as env_reward reduces it
    int c = 0;
    double s1 = 0.0, s2 = 0.0;
    Crossed o = {win_crossing(q, lo, hi, flip, c, s1, s2), 0u, 0.0, 0.0};
    if (o.any) {
      o.c = wave_sum_u32((unsigned)c);
      o.s1 = wave_sum_f64(s1);
      o.s2 = wave_sum_f64(s2);
    }
    return o;
  }
};
struct FormHWin {     // two envs per wavefront
  using Win = HWin;
  static constexpr int LPE = 32, KPL = 2;
  static constexpr bool HAS_ON = true;
  __device__ static Win make(const unsigned (&k)[2], int r0, int hi) { return HWin{k[0], k[1], r0, hi}; }
  __device__ static void keys(const Win& q, unsigned (&k)[2]) { k[0] = q.a; k[1] = q.b; }
  __device__ static bool update(Win& q, unsigned xn, unsigned xo, bool has_old, int n_prev, bool on, int e, int l) {
    return sdc_hw::hw_update(q, xn, xo, has_old, n_prev, on, e, l);
  }
  __device__ static bool resolve(const Win& q, int k, int n, int e, unsigned& a, unsigned& b) { return sdc_hw::hw_resolve(q, k, n, e, a, b); }
  __device__ static unsigned spans(const Win& q, unsigned lo, unsigned hi, int n, int e) { return sdc_hw::hw_spans(q, lo, hi, n, e) ? 1u : 0u; }
  __device__ static unsigned first(const Win& q, int e) { return sdc_hw::win_first(q, e); }
  __device__ static unsigned last(const Win& q, int e) { return sdc_hw::win_last(q, e); }
  __device__ static Crossed crossed(const Win& q, unsigned lo, unsigned hi, unsigned flip, bool en) {   // as pair_reward_fast reduces it
    const bool x = en && sdc_hw::win_any_in(q, lo, hi);
    unsigned cl;
    double s1l, s2l;
    sdc_hw::win_crossed(q, lo, hi, flip, en, cl, s1l, s2l);
    return Crossed{sdc_hw::half_sum_u32(x ? 1u : 0u) != 0u, sdc_hw::half_sum_u32(cl), half_sum_f64(s1l), half_sum_f64(s2l)};
  }
};
struct FormQWin {     // four envs per wavefront
  using Win = QWin;
  static constexpr int LPE = 16, KPL = 4;
  static constexpr bool HAS_ON = true;
  __device__ static Win make(const unsigned (&k)[4], int r0, int hi) { return QWin{k[0], k[1], k[2], k[3], r0, hi}; }
  __device__ static void keys(const Win& q, unsigned (&k)[4]) { k[0] = q.k0; k[1] = q.k1; k[2] = q.k2; k[3] = q.k3; }
  __device__ static bool update(Win& q, unsigned xn, unsigned xo, bool has_old, int n_prev, bool on, int e, int l) {
    return sdc_hw::hw_update(q, xn, xo, has_old, n_prev, on, e, l);
  }
  __device__ static bool resolve(const Win& q, int k, int n, int e, unsigned& a, unsigned& b) { return sdc_hw::hw_resolve(q, k, n, e, a, b); }
  // (the quad mapping has no spans function: pair_reward_fast tests the cached first / last keys, which are emitted instead)
  __device__ static unsigned spans(const Win&, unsigned, unsigned, int, int) { return NOT_APPLICABLE; }
  __device__ static unsigned first(const Win& q, int e) { return sdc_hw::win_first(q, e); }
  __device__ static unsigned last(const Win& q, int e) { return sdc_hw::win_last(q, e); }
  __device__ static Crossed crossed(const Win& q, unsigned lo, unsigned hi, unsigned flip, bool en) {
    const bool x = en && sdc_hw::win_any_in(q, lo, hi);
    unsigned cl;
    double s1l, s2l;
    sdc_hw::win_crossed(q, lo, hi, flip, en, cl, s1l, s2l);
    return Crossed{sdc_hw::row_sum_u32(x ? 1u : 0u) != 0u, sdc_hw::row_sum_u32(cl), sdc_hw::row_sum_f64(s1l), sdc_hw::row_sum_f64(s2l)};
  }
};

template <class F>
__global__ __launch_bounds__(64) void ops_kernel(const OpsArgs A) {
  constexpr int LPE = F::LPE, KPL = F::KPL, SLOTS = 64 / LPE;
  const int lane = (int)threadIdx.x, e = lane / LPE, l = lane % LPE;
  const int slot_raw = (int)blockIdx.x * SLOTS + e;
  const bool live = slot_raw < A.S;                 // (a slot past the end runs on the last slot's input with `on` false and stores nothing)
  const size_t slot = (size_t)(live ? slot_raw : A.S - 1);
  unsigned k[KPL];
#pragma unroll
  for (int j = 0; j < KPL; j++) k[j] = A.keys0[slot * 64 + KPL * l + j];
  const int* mt = A.meta + slot * 4;
  typename F::Win q = F::make(k, mt[0], mt[1]);
  int n = mt[2];
  const bool on = F::HAS_ON ? (live && mt[3] != 0) : true;
#pragma unroll 1
  for (int t = 0; t < A.T; t++) {
    const size_t st = slot * A.T + t;
    const unsigned* op = A.ops + st * 4;
    const unsigned* iv = A.iv + st * 4;
    const bool has_old = op[2] != 0u;
    const bool ch = F::update(q, op[0], op[1], has_old, n, on, e, l);
    if (on && !has_old) n += 1;
    int k1, k3;
    quartile_ranks(n, k1, k3);
    unsigned a1 = 0u, b1 = 0u, a3 = 0u, b3 = 0u;
    const bool ok1 = F::resolve(q, k1, n, e, a1, b1), ok3 = F::resolve(q, k3, n, e, a3, b3);
    const unsigned sp0 = F::spans(q, iv[0], iv[1], n, e), sp1 = F::spans(q, iv[2], iv[3], n, e);
    const unsigned wf = F::first(q, e), wl = F::last(q, e);
    const Crossed x0 = F::crossed(q, iv[0], iv[1], 0u, on), x1 = F::crossed(q, iv[2], iv[3], KEY_NONE, on);
    if (live) {
      F::keys(q, k);
#pragma unroll
      for (int j = 0; j < KPL; j++) A.okeys[st * 64 + KPL * l + j] = k[j];
      if (l == 0) {
        unsigned* o = A.oi + st * OI;
        o[OI_R0] = (unsigned)q.r0; o[OI_HI] = (unsigned)q.hi; o[OI_CH] = ch ? 1u : 0u;
        o[OI_OK1] = ok1 ? 1u : 0u; o[OI_A1] = a1; o[OI_B1] = b1;
        o[OI_OK3] = ok3 ? 1u : 0u; o[OI_A3] = a3; o[OI_B3] = b3;
        o[OI_SPAN0] = sp0; o[OI_SPAN1] = sp1;
        o[OI_ANY0] = x0.any ? 1u : 0u; o[OI_C0] = x0.c; o[OI_ANY1] = x1.any ? 1u : 0u; o[OI_C1] = x1.c;
        o[OI_FIRST] = wf; o[OI_LAST] = wl; o[OI_N] = (unsigned)n;
        o[18] = 0u; o[19] = 0u;
        double* d = A.od + st * 4;
        d[0] = x0.s1; d[1] = x0.s2; d[2] = x1.s1; d[3] = x1.s2;
      }
    }
  }
}

// ---- bounds: in [5][n] = n, a1, b1, a3, b3; out od[3][n] = lb, ub, ctr; ou[2][n] = klb, kub ---------------------------------------------------
__global__ __launch_bounds__(256) void bounds_kernel(const unsigned* __restrict__ in, double* __restrict__ od, unsigned* __restrict__ ou,
                                                     const int n) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  const size_t N = (size_t)n;
  const Bounds b = clip_bounds((int)in[i], in[N + i], in[2 * N + i], in[3 * N + i], in[4 * N + i]);
  od[i] = b.lb; od[N + i] = b.ub; od[2 * N + i] = b.ctr;
  ou[i] = b.klb; ou[N + i] = b.kub;
}

// ---- moments: in ni[2][n] = n, n_full; d[7][n] = lb, ub, A1, A2, T1, T2, 1 / n_full; out [3][n] = mean, sd, inv_sd ------------------------------
// (n == n_full takes the reciprocal form of the two divisions, as a full ring does; any other n_full the plain quotient)
__global__ __launch_bounds__(256) void moments_kernel(const int* __restrict__ ni, const double* __restrict__ d, double* __restrict__ out,
                                                      const int n) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  const size_t N = (size_t)n;
  const Bounds b = {d[i], d[N + i], 0.0, 2u, 2u};
  double mean, sd, inv_sd;
  const int nf = ni[N + i];
  clipped_moments(ni[i], b, d[2 * N + i], d[3 * N + i], d[4 * N + i], d[5 * N + i], mean, sd, inv_sd, nf, d[6 * N + i], (double)nf);
  out[i] = mean; out[N + i] = sd; out[2 * N + i] = inv_sd;
}

// ---- refill / refill_coop ----------------------------------------------------------------------------------------------------------------------
// in  ring[case][SDC_HIST_STRIDE], win[case][64], meta[case][8] = r0, hi, dir, k, n, patch_slot, patch_x, side
// out okeys[case][NW][64], om[case][NW][2] = r0, hi   (NW = 1; refill_coop: 4, the window as each wavefront returns it)
enum { RM_R0 = 0, RM_HI, RM_DIR, RM_K, RM_N, RM_PSLOT, RM_PX, RM_SIDE, RM = 8 };
struct RefillArgs {
  const unsigned* ring;
  const unsigned* win;
  const int* meta;
  unsigned* okeys;
  int* om;
};
template <int BATCH>
__global__ __launch_bounds__(64) void refill_kernel(const RefillArgs A) {
  __shared__ TailLds tl;
  const int lane = (int)threadIdx.x;
  const size_t c = blockIdx.x;
  const int* m = A.meta + c * RM;
  QTrack q = {A.win[c * 64 + lane], m[RM_R0], m[RM_HI]};
  const RingView R = {reinterpret_cast<const uint4*>(A.ring + c * SDC_HIST_STRIDE), m[RM_PSLOT], (unsigned)m[RM_PX]};
  qt_refill<BATCH>(q, m[RM_DIR], m[RM_K], m[RM_N], R, lane, tl, (unsigned)m[RM_SIDE]);
  A.okeys[c * 64 + lane] = q.w;
  if (lane == 0) {
    A.om[c * 2] = q.r0;
    A.om[c * 2 + 1] = q.hi;
  }
}
__global__ __launch_bounds__(64 * COOP_NW) void refill_coop_kernel(const RefillArgs A) {
  __shared__ CoopLds cl;
  const int lane = (int)threadIdx.x % 64, wave = (int)threadIdx.x / 64;
  const size_t c = blockIdx.x;
  const int* m = A.meta + c * RM;
  QTrack q = {A.win[c * 64 + lane], m[RM_R0], m[RM_HI]};
  const RingView R = {reinterpret_cast<const uint4*>(A.ring + c * SDC_HIST_STRIDE), m[RM_PSLOT], (unsigned)m[RM_PX]};
  qt_refill_coop(q, m[RM_DIR], m[RM_K], m[RM_N], R, lane, wave, cl, (unsigned)m[RM_SIDE]);
  A.okeys[(c * COOP_NW + wave) * 64 + lane] = q.w;
  if (lane == 0) {
    A.om[(c * COOP_NW + wave) * 2] = q.r0;
    A.om[(c * COOP_NW + wave) * 2 + 1] = q.hi;
  }
}

// ---- rebuild: in ring, meta[case][4] = n, patch_slot, patch_x, -; out okeys[case][4][64] = q1, q3, bu, bl; oi[case][16]; od[case][12] -------
enum { RB_Q1 = 0, RB_Q3 = 2, RB_BU = 4, RB_BL = 6, RB_QC = 8, RB_KLB = 10, RB_KUB, RB_OK, RB_I = 16 };
enum { RB_A1 = 0, RB_A2, RB_QS1, RB_QS2 = 4, RB_MEAN = 6, RB_SD, RB_LB, RB_UB, RB_CTR, RB_D = 12 };
__global__ __launch_bounds__(64) void rebuild_kernel(const unsigned* __restrict__ ring, const int* __restrict__ meta,
                                                     unsigned* __restrict__ okeys, int* __restrict__ oi, double* __restrict__ od) {
  __shared__ TailLds tl;
  const int lane = (int)threadIdx.x;
  const size_t c = blockIdx.x;
  const int* m = meta + c * 4;
  const RingView R = {reinterpret_cast<const uint4*>(ring + c * SDC_HIST_STRIDE), m[1], (unsigned)m[2]};
  const Rebuilt o = rebuild_state(R, lane, m[0], tl);
  unsigned* k = okeys + c * 4 * 64 + lane;
  k[0] = o.q1.hi > 0 ? o.q1.w : KEY_NONE;      // (a window that was not built has no keys: its register was never written)
  k[64] = o.q3.hi > 0 ? o.q3.w : KEY_NONE;
  k[128] = o.bu.hi > 0 ? o.bu.w : KEY_NONE;
  k[192] = o.bl.hi > 0 ? o.bl.w : KEY_NONE;
  if (lane == 0) {
    int* i = oi + c * RB_I;
    i[RB_Q1] = o.q1.hi > 0 ? o.q1.r0 : 0; i[RB_Q1 + 1] = o.q1.hi;
    i[RB_Q3] = o.q3.hi > 0 ? o.q3.r0 : 0; i[RB_Q3 + 1] = o.q3.hi;
    i[RB_BU] = o.bu.hi > 0 ? o.bu.r0 : 0; i[RB_BU + 1] = o.bu.hi;
    i[RB_BL] = o.bl.hi > 0 ? o.bl.r0 : 0; i[RB_BL + 1] = o.bl.hi;
    i[RB_QC] = o.qc[0]; i[RB_QC + 1] = o.qc[1];
    i[RB_KLB] = (int)o.b.klb; i[RB_KUB] = (int)o.b.kub; i[RB_OK] = o.ok ? 1 : 0;
    i[13] = i[14] = i[15] = 0;
    double* d = od + c * RB_D;
    d[RB_A1] = o.A1; d[RB_A2] = o.A2;
    d[RB_QS1] = o.qs1[0]; d[RB_QS1 + 1] = o.qs1[1]; d[RB_QS2] = o.qs2[0]; d[RB_QS2 + 1] = o.qs2[1];
    d[RB_MEAN] = o.mean; d[RB_SD] = o.sd; d[RB_LB] = o.b.lb; d[RB_UB] = o.b.ub; d[RB_CTR] = o.b.ctr;
    d[11] = 0.0;
  }
}

// ---- bisect_build: in ring, meta[case][8] = n, A1, B1, A3, B3, -; out ok4[case][4] = the keys at those ranks; okeys[case][2][64]; oi[case][4]
__global__ __launch_bounds__(64) void bisect_build_kernel(const unsigned* __restrict__ ring, const int* __restrict__ meta,
                                                          unsigned* __restrict__ ok4, unsigned* __restrict__ okeys, int* __restrict__ oi) {
  __shared__ TailLds tl;
  const int lane = (int)threadIdx.x;
  const size_t c = blockIdx.x;
  const int* m = meta + c * 8;
  const RingView R = {reinterpret_cast<const uint4*>(ring + c * SDC_HIST_STRIDE), -1, 0u};
  const Keys4 kv = wave_bisection4(R, lane, m[1], m[2], m[3], m[4]);
  QTrack q1, q3;
  windows_build(R, lane, kv, m[1], m[2], m[3], m[4], tl, q1, q3);
  okeys[c * 128 + lane] = q1.w;
  okeys[c * 128 + 64 + lane] = q3.w;
  if (lane == 0) {
    for (int j = 0; j < 4; j++) ok4[c * 4 + j] = kv.v[j];
    oi[c * 4] = q1.r0; oi[c * 4 + 1] = q1.hi; oi[c * 4 + 2] = q3.r0; oi[c * 4 + 3] = q3.hi;
  }
}

template <class F>
int launch_ops(const unsigned* keys0, const int* meta, const unsigned* ops, const unsigned* iv, unsigned* okeys, unsigned* oi, double* od,
               const int S, const int T, hipStream_t stream) {
  if (S <= 0 || T <= 0) return (int)hipSuccess;
  constexpr int SLOTS = 64 / F::LPE;
  const OpsArgs A = {keys0, meta, ops, iv, okeys, oi, od, S, T};
  hipLaunchKernelGGL((ops_kernel<F>), dim3((unsigned)((S + SLOTS - 1) / SLOTS)), dim3(64), 0, stream, A);
  return (int)hipGetLastError();
}
inline dim3 per_thread_grid(const int n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

extern "C" {
int probe_keys(const unsigned* in, unsigned* out, int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(keys_kernel, per_thread_grid(n), dim3(256), 0, stream, in, out, n);
  return (int)hipGetLastError();
}
int probe_reduce(const unsigned* u, const double* d, unsigned* ou, double* od, int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)n), dim3(64), 0, stream, u, d, ou, od);
  return (int)hipGetLastError();
}
int probe_window_ops_qtrack(const unsigned* keys0, const int* meta, const unsigned* ops, const unsigned* iv, unsigned* okeys, unsigned* oi,
                            double* od, int T, int S, hipStream_t stream) {
  return launch_ops<FormQTrack>(keys0, meta, ops, iv, okeys, oi, od, S, T, stream);
}
int probe_window_ops_hwin(const unsigned* keys0, const int* meta, const unsigned* ops, const unsigned* iv, unsigned* okeys, unsigned* oi,
                          double* od, int T, int S, hipStream_t stream) {
  return launch_ops<FormHWin>(keys0, meta, ops, iv, okeys, oi, od, S, T, stream);
}
int probe_window_ops_qwin(const unsigned* keys0, const int* meta, const unsigned* ops, const unsigned* iv, unsigned* okeys, unsigned* oi,
                          double* od, int T, int S, hipStream_t stream) {
  return launch_ops<FormQWin>(keys0, meta, ops, iv, okeys, oi, od, S, T, stream);
}
int probe_bounds(const unsigned* in, double* od, unsigned* ou, int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(bounds_kernel, per_thread_grid(n), dim3(256), 0, stream, in, od, ou, n);
  return (int)hipGetLastError();
}
int probe_moments(const int* ni, const double* d, double* out, int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(moments_kernel, per_thread_grid(n), dim3(256), 0, stream, ni, d, out, n);
  return (int)hipGetLastError();
}
int probe_refill5(const unsigned* ring, const unsigned* win, const int* meta, unsigned* okeys, int* om, int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(refill_kernel<5>, dim3((unsigned)n), dim3(64), 0, stream, RefillArgs{ring, win, meta, okeys, om});
  return (int)hipGetLastError();
}
int probe_refill10(const unsigned* ring, const unsigned* win, const int* meta, unsigned* okeys, int* om, int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(refill_kernel<10>, dim3((unsigned)n), dim3(64), 0, stream, RefillArgs{ring, win, meta, okeys, om});
  return (int)hipGetLastError();
}
int probe_refill_coop(const unsigned* ring, const unsigned* win, const int* meta, unsigned* okeys, int* om, int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(refill_coop_kernel, dim3((unsigned)n), dim3(64 * COOP_NW), 0, stream, RefillArgs{ring, win, meta, okeys, om});
  return (int)hipGetLastError();
}
int probe_rebuild(const unsigned* ring, const int* meta, unsigned* okeys, int* oi, double* od, int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(rebuild_kernel, dim3((unsigned)n), dim3(64), 0, stream, ring, meta, okeys, oi, od);
  return (int)hipGetLastError();
}
int probe_bisect_build(const unsigned* ring, const int* meta, unsigned* ok4, unsigned* okeys, int* oi, int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  hipLaunchKernelGGL(bisect_build_kernel, dim3((unsigned)n), dim3(64), 0, stream, ring, meta, ok4, okeys, oi);
  return (int)hipGetLastError();
}
}
