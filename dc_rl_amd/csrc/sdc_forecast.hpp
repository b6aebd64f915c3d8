// sdc_forecast.hpp -- what the plan calls (sdc_capi.hip plan_session) and sdc_forecast_traces hand to the two kernels of
// sdc_forecast.hip while a plan forecast is set on the handle (sdc_set_plan_forecast; the contract: include/sustaindc_hip.h).  Both
// plans go by value.
//
// A forecast is fc[j][n][c], fp64, j = 0 .. K + 1, c = (W, C, T, WB): what the planner believes trace c of env n is j table indices
// ahead.  sdc_forecast_fill_kernel writes it from every env's own record; sdc_forecast_swap_kernel overlays it on the step-input
// slots of the env's feature rows rel + 1 .. rel + K and keeps the bits it overwrites, 12 dwords per env-step:
//   [0, 1] W   [2] T1   [3] the env's rel   [4, 5] C   [6, 7] T   [8, 9] WB   [10, 11] NCNEXT
// so that the way back is a copy of saved bits into the rows the saved rel names, wherever the env stands by then.
#pragma once

#include <hip/hip_runtime.h>

#include "sdc_device.hpp"

enum { SDC_FC_W = 0, SDC_FC_C, SDC_FC_T, SDC_FC_WB, SDC_FC_CHANNELS };
#define SDC_FORECAST_SAVED_DWORDS 12
#define SDC_FORECAST_BLOCK 256
#define SDC_FORECAST_DAY 96        // table indices per day

// the 16-byte units of a feature row that hold a step-input slot of channel c
static_assert(SDC_FEAT_W == 10 && SDC_FEAT_T1 == 12 && SDC_FEAT_C == 22 && SDC_FEAT_T == 24 && SDC_FEAT_WB == 28 && SDC_FEAT_NCNEXT == 30 &&
                  SDC_FEAT_ROW == 32,
              "the unit of every slot below, and the dwords of the saved bits");
constexpr unsigned SDC_FC_UNIT_W = 2, SDC_FC_UNIT_T1 = 3, SDC_FC_UNIT_C = 5, SDC_FC_UNIT_T = 6, SDC_FC_UNIT_WB_NC = 7;
inline unsigned sdc_forecast_units(const unsigned channels) {      // bit c of `channels`: channel c is not PERFECT
  unsigned u = 0;
  if (channels & (1u << SDC_FC_W)) u |= 1u << SDC_FC_UNIT_W;
  if (channels & (1u << SDC_FC_C)) u |= (1u << SDC_FC_UNIT_C) | (1u << SDC_FC_UNIT_WB_NC);
  if (channels & (1u << SDC_FC_T)) u |= (1u << SDC_FC_UNIT_T) | (1u << SDC_FC_UNIT_T1);
  if (channels & (1u << SDC_FC_WB)) u |= 1u << SDC_FC_UNIT_WB_NC;
  return u;
}

struct SdcForecastFill {
  int n_envs, n_entries, table_len, lw;
  int mode_w, mode_c, mode_t, mode_wb;      // SDC_FORECAST_*
  const unsigned* rec;                      // [N][SDC_REC_DWORDS]
  const double *tabW, *tabC;                // [n_loc][table_len]
  const double *t_win, *wb_win;             // [N][lw]
  const double* values;                     // [>= n_entries][N][4], read by VALUES channels only
  double* fc;                               // [n_entries][N][4]
};

struct SdcForecastSwap {
  int n_envs, n_steps, n_rows;      // n_rows: feature rows per env (episode_steps + 1)
  int back;                         // 0: overlay and save; 1: put the saved bits back
  unsigned channels, units;         // bit c: channel c is overlaid; bit u: unit u of a row holds one of its slots (sdc_forecast_units)
  const unsigned* rec;
  const double* fc;                 // [n_steps + 2][N][4]
  float* feat;                      // SdcDev::feat
  unsigned* saved;                  // [n_steps][N][SDC_FORECAST_SAVED_DWORDS]
};

hipError_t sdc_forecast_fill_launch(const SdcForecastFill& F, hipStream_t st);
hipError_t sdc_forecast_swap_launch(const SdcForecastSwap& W, hipStream_t st);
