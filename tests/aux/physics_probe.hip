// physics_probe.hip -- TEST INFRASTRUCTURE: the step's shared arithmetic (dc_rl_amd/csrc/sdc_physics.hpp, sdc_device.hpp), one function per
// kernel, one input element per thread, so that tests/test_gpu_physics_functions.py can compare each function with a high-precision
// reference over its whole domain.  This file includes the product's header itself and restates none of its expressions; what it adds is
// the plumbing the step kernels have around them (operands from memory, results to memory) and, for the rack model, the one line with
// which both callers form a RackEnv from the config scalars and the load (sdc_pairstep.hpp dynamics, sdc_wide.hip).
//
// Every kernel exists twice: with the constants as literals (KLit, the general step kernels) and from a table in LDS (KLds, the
// specialised ones), filled per wavefront with ktab_fetch / ktab_store as the step kernels fill theirs.
//
// Launchers: int probe_<name>(int lds, const double* in, double* out, int n, hipStream_t stream); `in` is [n_in][n], `out` is
// [n_out][n] (row k of element i at k * n + i; integers and flags travel as doubles); returns the hipError_t of the launch.
// Built by tests/physics_probe.py with the library's compiler flags; nothing in dc_rl_amd/ knows about it.
#include "../../dc_rl_amd/csrc/sdc_physics.hpp"

namespace {

constexpr int PROBE_BLOCK = 256;

template <class KT>
struct KSource;
template <>
struct KSource<KLit> {
  static constexpr int lds_doubles = 1;
  __device__ static __forceinline__ KLit get(double*) { return KLit{}; }
};
template <>
struct KSource<KLds> {
  static constexpr int lds_doubles = SDC_K_LDS;
  // (every wavefront of the block writes the same values, as in the step kernels: the wavefront's own synchronisation is enough)
  __device__ static __forceinline__ KLds get(double* tab) {
    const int lane = (int)(threadIdx.x % SDC_WAVE);
    double k0, k1;
    ktab_fetch(lane, k0, k1);
    ktab_store(tab, lane, k0, k1);
    wave_sync();
    return KLds{tab};
  }
};

// in(k) / out(k): row k of this thread's element
struct Rows {
  const double* __restrict__ in;
  double* __restrict__ out;
  int n, i;
  __device__ __forceinline__ double operator()(const int k) const { return in[(size_t)k * n + i]; }
  __device__ __forceinline__ void put(const int k, const double v) const { out[(size_t)k * n + i] = v; }
};

template <class KT, class F>
__global__ __launch_bounds__(PROBE_BLOCK) void probe_kernel(const double* __restrict__ in, double* __restrict__ out, const int n) {
  __shared__ double tab[KSource<KT>::lds_doubles];
  const KT kt = KSource<KT>::get(tab);          // (before the bounds check: whole wavefronts fill the table)
  const int i = (int)(blockIdx.x * PROBE_BLOCK + threadIdx.x);
  if (i >= n) return;
  F::run(kt, Rows{in, out, n, i});
}

template <class F>
int probe_launch(const int lds, const double* in, double* out, const int n, hipStream_t stream) {
  if (n <= 0) return (int)hipSuccess;
  const dim3 grid((unsigned)((n + PROBE_BLOCK - 1) / PROBE_BLOCK)), block(PROBE_BLOCK);
  if (lds)
    hipLaunchKernelGGL((probe_kernel<KLds, F>), grid, block, 0, stream, in, out, n);
  else
    hipLaunchKernelGGL((probe_kernel<KLit, F>), grid, block, 0, stream, in, out, n);
  return (int)hipGetLastError();
}

// ---- the short transcendentals ---------------------------------------------------------------------------------------------------------
struct FLog2 {      // in: x                      out: log2 x
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) { r.put(0, log2_pos_normal(r(0), kt)); }
};
struct FExp2Plain { // in: y                      out: 2^y
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) { r.put(0, exp2_plain(r(0), kt)); }
};
struct FExpPlain {  // in: t                      out: e^t
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) { r.put(0, exp_plain(r(0), kt)); }
};
struct FExp2Short { // in: y                      out: 2^y (degree 8)
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) { r.put(0, exp2_short(r(0), kt)); }
};
// in: P, V    out: rack_outlet at inlet 0, k_outlet 1 = P^1.096 / V^0.824 + (-14.01), formed by the header's own rack_outlet
struct FRise {
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) {
    RackEnv E = {};
    E.k_outlet = 1.0;
    r.put(0, rack_outlet(kt, E, 0.0, log2_pos_normal(r(0), kt), log2_pos_normal(r(1), kt)));
  }
};

// ---- the two division shortcuts ----------------------------------------------------------------------------------------------------------
struct FDivConst {  // in: x, c, 1 / c            out: x / c
  template <class KT>
  __device__ static void run(const KT, const Rows r) { r.put(0, sdc_div_const(r(0), r(1), r(2))); }
};
struct FDivFast {   // in: a, b                   out: a / b
  template <class KT>
  __device__ static void run(const KT, const Rows r) { r.put(0, sdc_div_fast(r(0), r(1))); }
};

// ---- chiller -----------------------------------------------------------------------------------------------------------------------------
struct FChiller {   // in: cap, load, ambient     out: power
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) { r.put(0, chiller_power(r(0), r(1), r(2), kt)); }
};

// ---- one rack ----------------------------------------------------------------------------------------------------------------------------
// in: m_cpu, c_cpu, rs_cpu, m_fan, c_fan, rs_fan, itfan_ref_p, rc_itfan_ref_v_ratio, it_fan_full_load_v, k_outlet,   (0..9: the config)
//     load_pct, stpt, r_n, r_supply, r_full, r_idle                                                                   (10..15)
// out: pc, pf, outlet, plain, inlet
template <class KT>
__device__ __forceinline__ RackEnv probe_rack_env(const KT kt, const Rows r) {
  const double load_pct = r(10);
  // (as both callers form it: the load's shifts of the CPU and fan curves)
  return RackEnv{r(0), r(1), r(3), r(4), r(2) * KDIV(load_pct, 100), r(5) * KDIV(load_pct, 20), r(6), r(7), r(8), r(9)};
}
struct FRackPoint {
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) {
    const RackEnv E = probe_rack_env(kt, r);
    double inlet;
    const RackOut o = rack_point(kt, E, r(12), r(13), r(14), r(15), r(11), inlet);
    r.put(0, o.pc); r.put(1, o.pf); r.put(2, o.out); r.put(3, o.plain ? 1.0 : 0.0); r.put(4, inlet);
  }
};
// the lane-per-env kernel's composition (sdc_wide.hip: the airflow's logarithm once per group of racks, selected per rack)
struct FRackWide {
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) {
    const RackEnv E = probe_rack_env(kt, r);
    const double r_n = r(12);
    const RackAir ra = rack_air(kt, E, r_n, r(13), r(11));
    const bool plain_v = rack_plain(kt, ra.vtot);
    const double l2v = log2_pos_normal(plain_v ? ra.vtot : 1.0, kt);
    const double pc = rack_cpu_power(ra, r_n, r(14), r(15));
    const double pw = pc + ra.pf;
    const bool plain = rack_plain(kt, pw) && plain_v;
    const double out = rack_outlet(kt, E, ra.inlet, log2_pos_normal(plain ? pw : 1.0, kt), plain ? l2v : 0.0);
    r.put(0, pc); r.put(1, ra.pf); r.put(2, out); r.put(3, plain ? 1.0 : 0.0); r.put(4, ra.inlet);
  }
};

// ---- HVAC + water ------------------------------------------------------------------------------------------------------------------------
// in: c_air, rho_air, ct_fan_ref_p, crac_supply_pu, rc_rho_air, rc_ctafr, p_it, avg_ret, stpt, amb, wet_bulb    out: comp, ct, water, total_kw
struct FHvac {
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) {
    const HvacPrm P = {r(0), r(1), r(2), r(3), r(4), r(5)};
    const HvacOut o = hvac_water(kt, P, r(6), r(7), r(8), r(9), r(10));
    r.put(0, o.comp); r.put(1, o.ct); r.put(2, o.water); r.put(3, o.total_kw);
  }
};

// ---- battery -----------------------------------------------------------------------------------------------------------------------------
// in: a_bat, bat_load, cap, 1 / cap, total_kw, ci        out: e_nobat, energy, co2, soc_after, bat_load after the step, fault mask
struct FBattery {
  template <class KT>
  __device__ static void run(const KT kt, const Rows r) {
    double bat_load = r(1);
    unsigned fault = 0u;
    const BatOut o = battery_step(kt, (int)r(0), bat_load, r(2), r(3), r(4), r(5), fault);
    r.put(0, o.e_nobat); r.put(1, o.energy); r.put(2, o.co2); r.put(3, o.soc_after); r.put(4, bat_load); r.put(5, (double)fault);
  }
};

}  // namespace

#define PROBE_LAUNCHER(NAME, F)                                                                                  \
  extern "C" int probe_##NAME(int lds, const double* in, double* out, int n, hipStream_t stream) {               \
    return probe_launch<F>(lds, in, out, n, stream);                                                             \
  }
PROBE_LAUNCHER(log2_pos_normal, FLog2)
PROBE_LAUNCHER(exp2_plain, FExp2Plain)
PROBE_LAUNCHER(exp_plain, FExpPlain)
PROBE_LAUNCHER(exp2_short, FExp2Short)
PROBE_LAUNCHER(rise, FRise)
PROBE_LAUNCHER(div_const, FDivConst)
PROBE_LAUNCHER(div_fast, FDivFast)
PROBE_LAUNCHER(chiller_power, FChiller)
PROBE_LAUNCHER(rack_point, FRackPoint)
PROBE_LAUNCHER(rack_wide, FRackWide)
PROBE_LAUNCHER(hvac_water, FHvac)
PROBE_LAUNCHER(battery_step, FBattery)
