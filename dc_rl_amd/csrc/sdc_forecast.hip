// sdc_forecast.hip -- the two kernels behind a plan forecast (the contract: include/sustaindc_hip.h sdc_set_plan_forecast; the plans
// and the layout of the saved bits: sdc_forecast.hpp).
//
// sdc_forecast_fill_kernel: one lane per (entry j, env n).  From the env's own record (cursor, episode step, trace set) it picks, per
// channel, the table index or window position its mode names, clamps it as sdc_features.hip does, and loads the value -- or takes
// the caller's.  Envs need not be in lock-step.  The window positions are at most rel + j, which the host holds below the window's
// length (n_entries <= steps left + 2, lw = episode_steps + 18); they are clamped to it all the same.
//
// sdc_forecast_swap_kernel: one lane per 16-byte unit of the rows rel + 1 .. rel + K of every env, consecutive lanes on consecutive
// units of a row and consecutive rows of a step (the rows of a lock-step batch are contiguous per step).  A lane whose unit holds
// no slot of an overlaid channel leaves at once.  Forward: load the unit, keep the slot dwords it is about to replace in the saved
// bits, replace them with the forecast's, store the unit.  Back: load the unit, put the saved dwords in, store it; the row is the one
// the saved rel names.  Nothing else writes the rows while a plan call runs, and the launches of one stream run in order, so the
// read-modify-write of a unit is exact.  A row index past the env's rows (which the host refuses beforehand) is not touched.
#include <hip/hip_runtime.h>

#include "sdc_device.hpp"
#include "sdc_forecast.hpp"
#include "sdc_rowcopy.hpp"

namespace {

__device__ __forceinline__ int clampi(const int x, const int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// the table index / window position of entry j under `mode`, from the env's own i / rel
__device__ __forceinline__ int table_index(const int mode, const int i, const int j) {
  if (mode == SDC_FORECAST_PERSISTENCE) return i;
  if (mode == SDC_FORECAST_DAILY && j >= 1) return i + j - SDC_FORECAST_DAY;
  return i + j;
}
__device__ __forceinline__ int window_index(const int mode, const int rel, const int j) {
  if (mode == SDC_FORECAST_PERSISTENCE) return rel;
  if (mode == SDC_FORECAST_DAILY && j >= 1) return rel + j >= SDC_FORECAST_DAY ? rel + j - SDC_FORECAST_DAY : rel;
  return rel + j;
}

// a double into two dwords of a unit (elements of a clang vector do not bind to references)
#define put_f64(lo, hi, value)            \
  do {                                    \
    const double d_ = (value);            \
    lo = (unsigned)__double2loint(d_);    \
    hi = (unsigned)__double2hiint(d_);    \
  } while (0)

}  // namespace

extern "C" __global__ void __launch_bounds__(SDC_FORECAST_BLOCK) sdc_forecast_fill_kernel(SdcForecastFill F) {
  const size_t t = (size_t)blockIdx.x * SDC_FORECAST_BLOCK + threadIdx.x;
  const size_t N = (size_t)F.n_envs;
  if (t >= (size_t)F.n_entries * N) return;
  const int j = (int)(t / N), n = (int)(t % N);
  const unsigned* const r = F.rec + (size_t)n * SDC_REC_DWORDS;
  const int i = (int)r[R_CURSOR], rel = (int)r[R_TREL], loc = (int)r[R_LOC];
  const size_t at = t * SDC_FC_CHANNELS;      // entry (j, n) of F.values and F.fc
  const size_t tab = (size_t)loc * (size_t)F.table_len, win = (size_t)n * (size_t)F.lw;
  const double w = F.mode_w == SDC_FORECAST_VALUES ? F.values[at + SDC_FC_W] : F.tabW[tab + clampi(table_index(F.mode_w, i, j), F.table_len - 1)];
  const double c = F.mode_c == SDC_FORECAST_VALUES ? F.values[at + SDC_FC_C] : F.tabC[tab + clampi(table_index(F.mode_c, i, j), F.table_len - 1)];
  const double tt = F.mode_t == SDC_FORECAST_VALUES ? F.values[at + SDC_FC_T] : F.t_win[win + clampi(window_index(F.mode_t, rel, j), F.lw - 1)];
  const double wb = F.mode_wb == SDC_FORECAST_VALUES ? F.values[at + SDC_FC_WB] : F.wb_win[win + clampi(window_index(F.mode_wb, rel, j), F.lw - 1)];
  double* const o = F.fc + at;
  o[SDC_FC_W] = w;
  o[SDC_FC_C] = c;
  o[SDC_FC_T] = tt;
  o[SDC_FC_WB] = wb;
}

extern "C" __global__ void __launch_bounds__(SDC_FORECAST_BLOCK) sdc_forecast_swap_kernel(SdcForecastSwap W) {
  constexpr unsigned ROW_UNITS = SDC_FEAT_ROW / 4;
  static_assert(ROW_UNITS == 8, "a lane's unit is the low three bits of its index");
  const size_t t = (size_t)blockIdx.x * SDC_FORECAST_BLOCK + threadIdx.x;
  const size_t N = (size_t)W.n_envs;
  const unsigned unit = (unsigned)(t & (ROW_UNITS - 1));
  const size_t es = t / ROW_UNITS;      // env-step: k * N + n
  if (es >= (size_t)W.n_steps * N || ((W.units >> unit) & 1u) == 0u) return;
  const int k = (int)(es / N), n = (int)(es % N);
  unsigned* const sv = W.saved + es * SDC_FORECAST_SAVED_DWORDS;
  const unsigned* const r = W.rec + (size_t)n * SDC_REC_DWORDS;
  const unsigned rel = W.back ? sv[3] : r[R_TREL];
  const unsigned row = rel + 1u + (unsigned)k;
  // (the lane of the first overlaid unit keeps the env's rel; it is the same lane in both directions, so it reads what it wrote)
  if (!W.back && unit == (unsigned)__builtin_ctz(W.units)) sv[3] = rel;
  if (row >= (unsigned)W.n_rows) return;
  u32x4* const p = reinterpret_cast<u32x4*>(W.feat + ((size_t)row * N + (size_t)n) * SDC_FEAT_ROW) + unit;
  u32x4 v = *p;
  const double* const fc = W.fc + es * SDC_FC_CHANNELS;      // entry k; entries k + 1, k + 2: N, 2 N rows further
  const size_t next = N * SDC_FC_CHANNELS;
  if (unit == SDC_FC_UNIT_W) {
    if (W.back) { v.z = sv[0]; v.w = sv[1]; }
    else { sv[0] = v.z; sv[1] = v.w; put_f64(v.z, v.w, fc[SDC_FC_W]); }
  } else if (unit == SDC_FC_UNIT_T1) {
    if (W.back) v.x = sv[2];
    else { sv[2] = v.x; v.x = __float_as_uint((float)fc[next + SDC_FC_T]); }
  } else if (unit == SDC_FC_UNIT_C) {
    if (W.back) { v.z = sv[4]; v.w = sv[5]; }
    else { sv[4] = v.z; sv[5] = v.w; put_f64(v.z, v.w, fc[SDC_FC_C]); }
  } else if (unit == SDC_FC_UNIT_T) {
    if (W.back) { v.x = sv[6]; v.y = sv[7]; }
    else { sv[6] = v.x; sv[7] = v.y; put_f64(v.x, v.y, fc[SDC_FC_T]); }
  } else {      // SDC_FC_UNIT_WB_NC: the wet bulb's slot, and the carbon intensity's normalised value two entries on
    if ((W.channels >> SDC_FC_WB) & 1u) {
      if (W.back) { v.x = sv[8]; v.y = sv[9]; }
      else { sv[8] = v.x; sv[9] = v.y; put_f64(v.x, v.y, fc[SDC_FC_WB]); }
    }
    if ((W.channels >> SDC_FC_C) & 1u) {
      if (W.back) { v.z = sv[10]; v.w = sv[11]; }
      else {
        sv[10] = v.z; sv[11] = v.w;
        const double ci_min = __hiloint2double((int)r[R_CI_MIN + 1], (int)r[R_CI_MIN]);
        const double ci_den = __hiloint2double((int)r[R_CI_DEN + 1], (int)r[R_CI_DEN]);
        put_f64(v.z, v.w, (fc[2 * next + SDC_FC_C] - ci_min) / ci_den);      // sdc_features.hip:123, 179
      }
    }
  }
  *p = v;
}

hipError_t sdc_forecast_fill_launch(const SdcForecastFill& F, hipStream_t st) {
  const size_t lanes = (size_t)F.n_entries * (size_t)F.n_envs;
  hipLaunchKernelGGL(sdc_forecast_fill_kernel, dim3((unsigned)((lanes + SDC_FORECAST_BLOCK - 1) / SDC_FORECAST_BLOCK)),
                     dim3(SDC_FORECAST_BLOCK), 0, st, F);
  return hipGetLastError();
}

hipError_t sdc_forecast_swap_launch(const SdcForecastSwap& W, hipStream_t st) {
  const size_t lanes = (size_t)W.n_steps * (size_t)W.n_envs * (SDC_FEAT_ROW / 4);
  hipLaunchKernelGGL(sdc_forecast_swap_kernel, dim3((unsigned)((lanes + SDC_FORECAST_BLOCK - 1) / SDC_FORECAST_BLOCK)),
                     dim3(SDC_FORECAST_BLOCK), 0, st, W);
  return hipGetLastError();
}
