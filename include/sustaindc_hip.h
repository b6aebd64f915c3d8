/*
 * sustaindc_hip.h -- C-ABI of the MI355X-native vectorised SustainDC step.
 *
 * One handle = N environment instances resident on ONE GPU.  All obs / action / reward / info
 * buffers are device memory owned by the caller (PyTorch-ROCm tensors in the Python host); the
 * library borrows the raw pointers for the duration of a call and owns only its internal
 * struct-of-arrays state, trace tables and history rings.  Launches are asynchronous on the
 * caller's HIP stream.  No torch types, no C++ types: plain pointers and sizes.
 *
 * The reference (HewlettPackard/dc-rl) is pure Python and has no FFI for this path; each entry
 * point below names the reference interface it replaces (file:line under /root/reference).
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Return value: 0 on success, negative on error; message via sdc_last_error().
 * Threading: one host thread per handle; one handle per GPU.
 */
#ifndef SUSTAINDC_HIP_H
#define SUSTAINDC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDC_MAX_RACKS 64
#define SDC_N_AGENTS 3
#define SDC_OBS_PAD 26       /* per-agent obs padded to 26 (harl/envs/sustaindc/harlsustaindc_env.py:25-26) */
#define SDC_SHARE_OBS_DIM 29 /* harlsustaindc_env.py:78-80 */
#define SDC_INFO_DIM 44
#define SDC_TABLE_LEN 35040  /* 365 d x 96 steps (utils/managers.py:184) */

/* info[N][SDC_INFO_DIM] columns; names are the reference's info keys
 * (envs/carbon_ls.py:291-308, envs/dc_gym.py:213-229, envs/bat_env_fwd_view.py:111-122,
 *  sustaindc_env.py:676-683) */
enum sdc_info_col {
  SDC_INFO_LS_ORIGINAL_WORKLOAD = 0,
  SDC_INFO_LS_SHIFTED_WORKLOAD,
  SDC_INFO_LS_TASKS_IN_QUEUE,
  SDC_INFO_LS_NORM_TASKS_IN_QUEUE,
  SDC_INFO_LS_TASKS_DROPPED,
  SDC_INFO_LS_TASKS_PROCESSED,
  SDC_INFO_LS_OLDEST_TASK_AGE,
  SDC_INFO_LS_AVERAGE_TASK_AGE,
  SDC_INFO_LS_OVERDUE_PENALTY,
  SDC_INFO_LS_COMPUTED_TASKS,
  SDC_INFO_LS_CURRENT_HOUR,
  SDC_INFO_LS_AGE_HIST0, SDC_INFO_LS_AGE_HIST1, SDC_INFO_LS_AGE_HIST2, SDC_INFO_LS_AGE_HIST3, SDC_INFO_LS_AGE_HIST4,
  SDC_INFO_DC_ITE_TOTAL_POWER_KW,
  SDC_INFO_DC_CT_TOTAL_POWER_KW,
  SDC_INFO_DC_COMPRESSOR_TOTAL_POWER_KW,
  SDC_INFO_DC_HVAC_TOTAL_POWER_KW,
  SDC_INFO_DC_TOTAL_POWER_KW,
  SDC_INFO_DC_CRAC_SETPOINT_DELTA,
  SDC_INFO_DC_CRAC_SETPOINT,
  SDC_INFO_DC_CPU_WORKLOAD_FRACTION,
  SDC_INFO_DC_INT_TEMPERATURE,
  SDC_INFO_DC_EXTERIOR_AMBIENT_TEMP,
  SDC_INFO_DC_WATER_USAGE,
  SDC_INFO_BAT_ACTION,
  SDC_INFO_BAT_SOC,
  SDC_INFO_BAT_CO2_FOOTPRINT,
  SDC_INFO_BAT_AVG_CI,
  SDC_INFO_BAT_TOTAL_ENERGY_WITHOUT_BATTERY_KWH,
  SDC_INFO_BAT_TOTAL_ENERGY_WITH_BATTERY_KWH,
  SDC_INFO_NORM_CI,
  SDC_INFO_OUTSIDE_TEMP,
  SDC_INFO_DAY,
  SDC_INFO_HOUR,
  SDC_INFO_FAULT,    /* bit mask, see SDC_FAULT_* (the reference raises / asserts instead) */
  SDC_INFO_ENERGY_Z, /* normalize_energy() output shared by the three rewards */
  SDC_INFO_RESERVED, /* diagnostic: how this step's reward normalisation was served: 0 incremental state only (no
                        history read), 1 a rank window was re-centred over the history inline, 2 incremental state
                        only and a window re-centred by a spare wavefront of the previous launch was taken over,
                        3 the state was rebuilt from the history, 5 a clip bound had left its window and the bounds' side
                        (tail sums, that window) was redone from the history (and, only with debug_flags bit 3: 4 incremental
                        state only and a re-centring request was filed).  Scheduling-dependent (which requests find
                        a free slot), unlike every other output */
  /* running return of the current episode INCLUDING this step (== the episode return on the done step);
   * feeds the return statistics the runners log (harl/common/base_logger.py:75-88) without host sums */
  SDC_INFO_EP_RETURN_LS,
  SDC_INFO_EP_RETURN_DC,
  SDC_INFO_EP_RETURN_BAT,
  SDC_INFO_EPISODE_STEP /* steps taken in the current episode, including this one */
};

#define SDC_FAULT_OUTLET_DELTA 1u  /* envs/datacenter.py:295-300 raises */
#define SDC_FAULT_CPU_LOAD 2u      /* envs/dc_gym.py:288-290 asserts */
#define SDC_FAULT_BAT_DISCHARGE 4u /* envs/bat_env_fwd_view.py:237 asserts */
#define SDC_FAULT_WORKLOAD 8u      /* envs/carbon_ls.py:333-336 raises */
#define SDC_FAULT_TABLE_RANGE 16u  /* cursor would leave the year table (reference: IndexError) */
#define SDC_FAULT_ACTION 64u       /* agent_dc / agent_bat action outside {0,1,2} (the reference's action_mapping /
                                      _action_to_direction lookups raise KeyError: envs/dc_gym.py:160, bat_env_fwd_view.py:99);
                                      the step treats it as "no change" / "idle".  agent_ls: any other value is "do
                                      nothing" in the reference too (envs/carbon_ls.py:266), flagged all the same */
#define SDC_FAULT_ORDER_STAT 32u   /* debug_flags bit 0: the incremental reward state disagreed with the exact recomputation */

typedef struct sdc_handle sdc_handle;

/* sdc_config.debug_flags, one name per bit the library reads.  Four kinds:
 *   PUBLIC MODE       changes what a call does, on any kernel;
 *   MEASUREMENT MODE  in-kernel diagnostics that only the general kernels carry: the call goes to the general step / rollout kernel
 *                     (they overwrite info[reserved] / the episode-return columns info[40..43]);
 *   MAPPING OVERRIDE  picks among the kernels that give the same results to the bit (csrc/sdc_dispatch.hpp: tests compare them);
 *   TEST HOOK         forces a path the tests could not otherwise reach.
 * A bit without a name sends the call to the general kernel as well. */
#define SDC_DEBUG_VERIFY 1           /* bit 0, PUBLIC MODE: after every sdc_step check the incremental reward state (the four rank
                                        windows, running sums) and the reported z-score against an exact bisection and a direct fp64
                                        pass over each env's history (slow; a mismatch sets SDC_FAULT_ORDER_STAT in info[fault],
                                        so sdc_step refuses a NULL info in this mode).  The multi-step entry points refuse it */
#define SDC_DEBUG_WHY_REBUILD 2      /* bit 1, MEASUREMENT MODE: info[reserved]'s path codes 3 / 5 carry why a rebuild happened */
#define SDC_DEBUG_PHASES 8           /* bit 3, MEASUREMENT MODE: per-wavefront phase durations in info[40..43], the rare paths the
                                        wavefront's step took in info[reserved] above bit 3 */
#define SDC_DEBUG_STAMPS 16          /* bit 4, MEASUREMENT MODE (with bit 3): absolute wavefront start / end stamps instead */
#define SDC_DEBUG_RECORD_WAIT 32     /* bit 5, MEASUREMENT MODE (with bit 3): info[40] = entry until the state record has arrived */
#define SDC_DEBUG_STEP_NO_ENV 64     /* bit 6, TEST HOOK: sdc_create reads the environment variable SDC_TEST_STEP_NO and starts the
                                        launch counter there (tests of the counter's wrap); the step does not see the bit */
#define SDC_DEBUG_GENERAL 128        /* bit 7, MAPPING OVERRIDE: always the GENERAL step / rollout kernels, never the ones
                                        specialised for the common case */
#define SDC_DEBUG_HW_ID 256          /* bit 8, MEASUREMENT MODE (with bit 3): info[40] = where the wavefront ran (XCC, SE, SH, CU,
                                        SIMD, wave) */
#define SDC_DEBUG_PAIR 512           /* bit 9, MAPPING OVERRIDE: the common-case kernels with two envs per wavefront whatever the
                                        batch size (by default four when the batch is a multiple of four and large: single steps
                                        above 5632 envs, the multi-step entry points above 4096) */
#define SDC_DEBUG_QUAD 1024          /* bit 10, MAPPING OVERRIDE: ... with four envs per wavefront whatever the size */
#define SDC_DEBUG_WIDE 2048          /* bit 11, MAPPING OVERRIDE: the lane-per-env kernel for any batch that is a multiple of 64 envs
                                        (by default from 7680 envs; sdc_rollout from 12288); sdc_create gives the batch the mirror
                                        the kernel reads.  Not together with bit 9 / 10 / 12: those win */
#define SDC_DEBUG_WIDE_OFF 4096      /* bit 12, MAPPING OVERRIDE: never the lane-per-env kernel */
#define SDC_DEBUG_BOUND_REPAIR 8192  /* bit 13, TEST HOOK (general kernel): every 61st (env + launch) redoes its clip bounds' side
                                        from the history as if a bound had left its window (a path ~4e-8 of the env-steps take by
                                        themselves) */
#define SDC_PLAN_DEBUG_TWO_STEPS 16384 /* bit 14, TEST HOOK: the handle's output block holds two steps, so that short horizons run
                                        the chunked path of sdc_plan / sdc_plan_cem / sdc_plan_cem_groups / sdc_rollout_stats; read by
                                        those calls alone, the step kernels never see the bit */

/* replaces: EnvConfig / SustainDC.__init__ wiring (sustaindc_env.py:34-160) for N envs */
typedef struct {
  int32_t n_envs;
  int32_t device;          /* HIP device ordinal */
  int32_t episode_steps;   /* days_per_episode * 96 (utils/managers.py:113) */
  int32_t hist_cap;        /* 10000 (utils/reward_creator.py:5) */
  int32_t queue_max_len;   /* 1000 (sustaindc_env.py:149) */
  int32_t n_locations;     /* number of trace-table sets */
  int32_t n_dc_configs;    /* number of data-centre parameter sets */
  int32_t auto_reset;      /* 1: reset finished envs inside sdc_step (harl/envs/env_wrappers.py:176-190) */
  uint64_t seed;           /* counter-based RNG seed for device-side resets */
  double weather_noise_std;   /* 0.75 (utils/managers.py:504) ; 0 disables the noise */
  double weather_noise_weight;/* 0.02 (utils/managers.py:504) */
  int32_t max_roll_days;   /* 14: roll in [0, 14) days (utils/managers.py:601) */
  int32_t debug_flags;     /* SDC_DEBUG_* below, or'ed; 0 in production */
  int32_t reward_method[3]; /* reward function per agent slot (ls, dc, bat), utils/reward_creator.py:322-334:
                               SDC_REWARD_DEFAULT the slot's own default_*_reward, SDC_REWARD_FOOTPRINT
                               default_dc_reward = default_bat_reward, SDC_REWARD_CUSTOM custom_agent_reward (0),
                               SDC_REWARD_TOU, SDC_REWARD_ENERGY_EFFICIENCY, SDC_REWARD_PUE, SDC_REWARD_WATER.
                               As in the reference only default_ls_reward appends to the energy history
                               (reward_creator.py:63): the history grows iff reward_method[0] == SDC_REWARD_DEFAULT */
  int32_t env_index_base;  /* global index of this batch's env 0 when the batch is one shard of a multi-GPU job: the
                              counter-based RNG of device-side resets is keyed on (seed, env_index_base + env, episode),
                              so a job draws the same start day / hour / roll / weather noise for global env i whatever
                              the number of GPUs it is sharded over (harl/utils/envs_tools.py:56-65 keys months and
                              seeds on the global rank the same way) */
  int32_t policy[3];       /* who chooses each agent slot's action (ls, dc, bat): SDC_POLICY_EXTERNAL the caller's
                              actions array; SDC_POLICY_DO_NOTHING the reference's base agents (utils/base_agents.py:
                              ls 1, dc 1, bat 2 -- what SustainDC plays for agents that are not trained,
                              sustaindc_env.py:172-191, :623-655); SDC_POLICY_RBC (bat slot) RBCBatteryAgent
                              (utils/rbc_agents.py:21-47, look_ahead 3, smooth_window 1); SDC_POLICY_TRIM_AND_RESPOND
                              (dc slot) trim_and_respond_ctrl (utils/trim_and_respond.py:8-38).  The policies run inside
                              the step kernel, so sdc_rollout can run closed-loop episodes without an action array. */
  int32_t reserved2;
  double trim_and_respond_limit; /* TandR_monitor_limit (27 in the reference), compared with the room temperature
                                    (dc_int_temperature) the previous step reported */
} sdc_config;

enum sdc_policy { SDC_POLICY_EXTERNAL = 0, SDC_POLICY_DO_NOTHING = 1, SDC_POLICY_RBC = 2, SDC_POLICY_TRIM_AND_RESPOND = 3 };

enum sdc_reward_method {
  SDC_REWARD_DEFAULT = 0,
  SDC_REWARD_FOOTPRINT = 1,
  SDC_REWARD_CUSTOM = 2,
  SDC_REWARD_TOU = 3,               /* DEVIATION: the reference indexes its price table with the float hour and raises
                                       KeyError off the full hour (reward_creator.py:191); here the hour is truncated */
  SDC_REWARD_ENERGY_EFFICIENCY = 4,
  SDC_REWARD_PUE = 5,
  SDC_REWARD_WATER = 6
};

/* replaces: DC_Config + Rack/CPU constants + sized HVAC values
 * (utils/dc_config_reader.py:39-145, envs/datacenter.py:31-135, utils/make_envs_pyenv.py:139-197) */
typedef struct {
  int32_t n_racks;
  int32_t reserved;
  double rack_n[SDC_MAX_RACKS];      /* CPUs per rack after the MAX_W_PER_RACK cap (datacenter.py:67-74) */
  double rack_full[SDC_MAX_RACKS];   /* full-load W per CPU */
  double rack_idle[SDC_MAX_RACKS];   /* idle W per CPU */
  double rack_supply[SDC_MAX_RACKS]; /* supply approach temperature, unclamped */
  double rack_return[SDC_MAX_RACKS]; /* return approach temperature */
  double m_cpu, c_cpu, rs_cpu;       /* datacenter.py:31-39 */
  double m_fan, c_fan, rs_fan;       /* datacenter.py:41-49 */
  double itfan_ref_p, itfan_ref_v_ratio, it_fan_full_load_v;
  double c_air, rho_air, crac_supply_pu;
  double ct_fan_ref_p, ctafr;        /* SIZED (make_envs_pyenv.py:159-161) */
  double min_temp, max_temp;         /* CRAC set-point clamp (make_envs_pyenv.py:125-126) */
  double init_setpoint;              /* 18 (make_envs_pyenv.py:124) */
  double bat_capacity_mwh;           /* sized battery capacity (sustaindc_env.py:152) */
} sdc_dc_params;

/* replaces: the (day, hour, roll, noise) draws of SustainDC.reset / Weather_Manager.reset
 * (sustaindc_env.py:454-461, utils/managers.py:581-628) when the caller wants to inject them
 * (parity tests).  All pointers are HOST memory, indexed by env. */
typedef struct {
  const int32_t* day;   /* [N] */
  const int32_t* hour;  /* [N] 0..23 */
  const double* ci_min; /* [N] min of C over [cursor, cursor+2880) (managers.py:435-437) */
  const double* ci_max;
  const double* t_min;  /* [N] same for the noised/rolled/clipped temperature (managers.py:606-608) */
  const double* t_max;
  const double* t_win;  /* [N][weather_window_len]: T[cursor0 + k] after noise+roll+clip */
  const double* wb_win; /* [N][weather_window_len]: wet bulb likewise */
  /* Alternative injection one level earlier (noise != NULL; ci_min .. wb_win are then ignored and may be NULL): the
   * draws of Weather_Manager.reset themselves -- the year's coherent-noise array as CoherentNoise.generate returned it
   * (managers.py:35-48) and the roll in days (:601) -- next to day / hour.  The device then does what it does after
   * its own draws: add the noise to the location's T / WB tables, roll, clip to [0, 45], take the 30-day min / max
   * from the cursor (managers.py:596-613) and the CI bounds (:435-437). */
  const double* noise;     /* [N][SDC_TABLE_LEN] or NULL */
  const int32_t* roll_days; /* [N], with noise */
} sdc_reset_override;

const char* sdc_last_error(void);
/* ABI version of this header: bumped whenever a struct layout or an entry point's arguments change.  sdc_version()
 * returns the value the library was BUILT with; a caller compares the two before anything else (dc_rl_amd/_lib.py
 * does) -- the .so is shipped out of band, so a stale one must fail loudly, not corrupt silently.
 *   100  round 1        300  sdc_config: env_index_base, policy[3], trim_and_respond_limit; sdc_reset_override: noise,
 *                            roll_days; sdc_rollout: actions_out; debug_flags bit 6
 *   310  sdc_set_actor, sdc_rollout_actor (closed loop with the actor networks inside the kernel); debug_flags bit 7
 *        (debug_flags bits 9 / 10 came later without a bump: no layout or argument list changed)
 *   312  sdc_state_layout
 *   313  sdc_clone_envs
 *        (sdc_snapshot_row_bytes, sdc_snapshot_envs, sdc_restore_envs came later without a bump: new entry points, no layout or
 *        existing argument list changed; sdc_mark_row_bytes, sdc_mark_envs, sdc_rewind_envs likewise; sdc_plan, sdc_plan_cem,
 *        sdc_rollout_stats and sdc_plan_cem_groups likewise; sdc_set_plan_terms and sdc_get_plan_terms likewise;
 *        sdc_set_plan_forecast, sdc_get_plan_forecast and sdc_forecast_traces likewise; sdc_rollout_actor_stats, sdc_rollout_cem_stats
 *        and sdc_rollout_cem_groups_stats likewise; sdc_set_critic, sdc_critic_values, sdc_set_plan_critic and sdc_get_plan_critic
 *        likewise; sdc_gae and sdc_action_log_probs likewise; sdc_actor_evaluate and sdc_ppo_terms likewise; sdc_critic_evaluate,
 *        sdc_value_loss and sdc_critic_backward likewise; sdc_actor_adam_step, sdc_critic_adam_step, sdc_get_actor, sdc_get_critic,
 *        sdc_get_actor_optim, sdc_set_actor_optim, sdc_get_critic_optim, sdc_set_critic_optim and sdc_set_critic_norm likewise) */
#define SDC_ABI_VERSION 313
int sdc_version(void);

int sdc_create(const sdc_config* cfg, sdc_handle** out);
int sdc_destroy(sdc_handle* h);

/* replaces: SustainDC.seed (sustaindc_env.py:241-251): re-key the counter-based RNG of device-side resets */
int sdc_set_seed(sdc_handle* h, uint64_t seed);

/* episode_steps + 18: samples of per-env weather the step can touch */
int sdc_weather_window_len(const sdc_handle* h);

/* replaces: Workload_Manager / CI_Manager / Weather_Manager table construction
 * (utils/managers.py:152-197, :318-388, :488-569).  Host arrays of length n (= SDC_TABLE_LEN):
 * W = cpu_smooth after scale_array + 16-tap smoothing (managers.py:268-271), C = carbon_smooth,
 * T / WB = interpolated dry / wet bulb BEFORE noise. */
int sdc_set_tables(sdc_handle* h, int loc_id, const double* W, const double* C, const double* T, const double* WB,
                   int n);

int sdc_set_dc_params(sdc_handle* h, int cfg_id, const sdc_dc_params* p);

/* per-env assignment (host arrays [N]): trace set, DC parameter set, and the inclusive range the
 * random start day is drawn from (sustaindc_env.py:198, :454) */
int sdc_assign_envs(sdc_handle* h, const int32_t* loc_id, const int32_t* cfg_id, const int32_t* day_lo,
                    const int32_t* day_hi);

/* replaces: SustainDC.reset (sustaindc_env.py:436-531) / ShareVecEnv.reset (env_wrappers.py:275-280).
 * mask_host: NULL = all envs, else [N] bytes (host).  ovr: NULL = draw on device.
 * obs [N][3][26] f32, share_obs [N][29] f32 (device; may be NULL).  A masked reset writes the masked envs' rows only.
 * Closed loop (sdc_set_actor): the library keeps its own copy of the latest observations; a reset with obs == NULL
 * invalidates it (sdc_rollout_actor then refuses until a reset / step has delivered observations), a masked reset
 * takes over the masked rows only (the other rows of the caller's buffer are not read). */
int sdc_reset(sdc_handle* h, const uint8_t* mask_host, const sdc_reset_override* ovr, float* obs, float* share_obs,
              void* stream);

/* replaces: SustainDC.step (sustaindc_env.py:533-621) + HARL adaptation + auto-reset
 * (harlsustaindc_env.py:106-131, env_wrappers.py:168-192) for all N envs.
 * actions [N][3] int32 (ls, dc, bat) in {0,1,2}; obs [N][3][26]; share_obs [N][29]; rew [N][3];
 * done [N] u8; info [N][SDC_INFO_DIM] f32; final_obs [N][3][26] receives the pre-reset observation of
 * envs that finished ("original_obs"); info / final_obs / share_obs may be NULL -- but in verify mode
 * (debug_flags SDC_DEBUG_VERIFY), whose check reads info[energy_z] and reports through info[fault]: there a NULL info
 * is refused. */
int sdc_step(sdc_handle* h, const int32_t* actions, float* obs, float* share_obs, float* rew, uint8_t* done,
             float* info, float* final_obs, void* stream);

/* n_steps env-steps in ONE launch for action sequences known up front (scripted / rule-based policies -- the
 * reference's utils/rbc_agents.py, utils/base_agents.py --, open-loop evaluation): every env advances n_steps times
 * without waiting for the others.  actions [n_steps][N][3]; obs [n_steps][N][3][26], share_obs [n_steps][N][29],
 * rew [n_steps][N][3], done [n_steps][N], info [n_steps][N][SDC_INFO_DIM] receive every step's outputs (share_obs /
 * info / final_obs may be NULL).  n_steps must not exceed sdc_steps_to_episode_end(); if it reaches the episode's
 * end and auto_reset is on, the finished envs are reset as in sdc_step (the last step's obs slice holds the reset
 * observation, final_obs [N][3][26] the pre-reset one).  Same results as n_steps calls of sdc_step.
 * Agent slots with a built-in policy (sdc_config.policy) ignore `actions`, which may be NULL when all three have one;
 * actions_out [n_steps][N][3] (device, or NULL) receives the actions every step applied. */
int sdc_rollout(sdc_handle* h, int n_steps, const int32_t* actions, float* obs, float* share_obs, float* rew,
                uint8_t* done, float* info, float* final_obs, int32_t* actions_out, void* stream);
/* CLOSED LOOP.  replaces: the actor forward pass of the reference's rollout loop (harl/runners/on_policy_base_runner.py
 * collect -> harl/algorithms/actors/on_policy_base.py get_actions -> StochasticPolicy.forward,
 * harl/models/policy_models/stochastic_policy.py:11-60) between two env steps: one agent's network
 *     LayerNorm(26) -> Linear(26, 64) -> act -> LayerNorm(64) -> Linear(64, 64) -> act -> LayerNorm(64) -> Linear(64, 3)
 * (harl/models/base/mlp.py:8-72, act.py:45-84; hidden_sizes [64, 64], happo.yaml:58) with the weights in torch's layout
 * ([out][in], row-major), fp32.  sdc_set_actor copies them to the device (host pointers). */
typedef struct {
  float ln0_gamma[26], ln0_beta[26];                 /* feature_norm (use_feature_normalization) */
  float w1[64 * 26], b1[64], ln1_gamma[64], ln1_beta[64];
  float w2[64 * 64], b2[64], ln2_gamma[64], ln2_beta[64];
  float w3[3 * 64], b3[3];                           /* act.action_out.linear */
  int32_t use_feature_normalization;                 /* 1: LayerNorm over the 26 inputs first */
  int32_t activation;                                /* 0 tanh, 1 relu */
} sdc_actor_params;
int sdc_set_actor(sdc_handle* h, int agent_slot, const sdc_actor_params* p);
/* n_steps env-steps in ONE launch, every step's three actions chosen INSIDE the kernel by the three actors from the
 * step's own observations (the first from the observations the last sdc_reset / sdc_step / sdc_rollout* call returned,
 * of which the library keeps a copy once an actor is set): observation -> actor -> action -> step without a launch or a
 * host round trip per step.  sample = 0: the distributions' mode (deterministic = True in the reference), 1: a draw
 * (counter-based RNG keyed on seed, global env index, the env's episode number, episode step and a stream constant, one word per
 * agent: THE POLICY HEAD below).  Outputs as sdc_rollout (all required but
 * final_obs); actions_out [n_steps][N][3] receives the actions, logits_out [n_steps][N][3][3] (may be NULL) the actors'
 * logits.  Only for the common case the specialised kernels serve (lock-step batch with feature rows, one data-centre
 * config of <= 32 racks, default rewards, an even number of envs) and three actors with the same activation; anything
 * else is refused.
 * THE POLICY HEAD: from an agent's three fp32 logits l0, l1, l2 -- the values logits_out receives -- to the action its env step is
 * given.  Both actor kernels (two and four envs per wavefront) do the same, and nothing but env state and configuration enters:
 * the same steps asked for in launches of other lengths, or by a shard of a larger job, choose the same actions.
 * MODE (sample = 0).  The first maximum: 1 if l1 > l0 and l1 >= l2, else 2 if l2 > l0 and l2 > l1, else 0 -- torch.argmax's rule,
 * ties towards the lower action.
 * DRAW (sample = 1).  One philox4x32_10 block per (env n, episode step) with counter (episode step, env_index_base + n, the env's
 * episode number, 0xAC70) and key (seed's low word, seed's high word).  The episode step counts from 0 at the env's reset (the batch
 * is in lock-step: one value per launched step); the episode number is the env's own -- 1 after its first reset, one more with every
 * reset or auto-reset, the "episode" state array -- so envs of one batch may differ in it; a launch never crosses an episode's end.
 * Words x, y, z serve agents ls, dc, bat, w is unused:  u = (float)(word >> 8) * 2^-24, in [0, 1) on a 24-bit grid.  Then, all fp32,
 * exp2 the hardware's (v_exp_f32, ~1 ulp), every other operation rounded once (there is no multiply-add pair to fuse):
 *   m = max(l0, l1, l2);  e_i = exp2((l_i - m) * log2 e), log2 e = 1.4426950408889634f;  t = u * ((e0 + e1) + e2);
 *   action = (t >= e0) + (t >= e0 + e1)
 * -- the inverse CDF of softmax(l); e2 enters the sum only.  An e_i that underflows to 0 is never drawn except by its place: l =
 * (-200, 0, -200) draws 1 for every u, u = 0 included.
 * NaN or infinite logits are not specified (torch's Categorical refuses them); finite weights and observations do not produce them:
 * a hidden layer whose activations are all equal (a dead ReLU layer) leaves its LayerNorm's beta, not a NaN. */
int sdc_rollout_actor(sdc_handle* h, int n_steps, int sample, float* obs, float* share_obs, float* rew, uint8_t* done,
                      float* info, float* final_obs, int32_t* actions_out, float* logits_out, void* stream);
/* steps until the first env finishes its episode (0: a reset is due) */
int sdc_steps_to_episode_end(const sdc_handle* h);
/* which envs finished their episode in the last sdc_step / sdc_rollout call -- the `done` output, but from the host's
 * mirror of the step counters (episodes have a fixed length), so a caller that keeps everything on the device learns
 * about episode boundaries (harl/envs/env_wrappers.py:176-190: "original_obs" bookkeeping) without a device->host
 * read.  Returns the number of finished envs; done_host [N] (host, may be NULL) is filled only when it is > 0. */
int sdc_last_done(const sdc_handle* h, uint8_t* done_host);
/* name of the kernel the last sdc_step / sdc_rollout / sdc_rollout_actor launched ("" before the first): the host picks by batch size and configuration
 * between the general kernel, the common-case kernels with two / four envs per wavefront and the lane-per-env kernel of the
 * largest batches (csrc/sdc_dispatch.hpp: the whole decision, and the table of kernels) -- all give the same results; tests and benchmarks name
 * what they measured with this.  The critic's two kernels (sdc_critic_values, THE PLAN CRITIC) are named here as well when they were
 * the last launch. */
const char* sdc_last_step_kernel(const sdc_handle* h);

/* parity injection + env checkpoint: copy one named state field to / from HOST memory, dense per env.
 * int32[N]:  cursor t_rel day hourq q_popped q_cum q_cumT q_head q_cum_hm1 q_cumT_hm1 last_delta consecutive
 *            scale hist_len hist_pos episode fault loc_id cfg_id day_lo day_hi hist_n
 * double[N]: stpt bat_load ci_min ci_den t_min t_den hist_ref
 * record (uint32[N][64], the raw 256-byte state records);  header (uint32[N][64], step hand-off + reward state);
 * qwin (uint32[N][64][4], the reward state's rank windows: per lane the keys of {Q1, Q3, upper bound, lower bound});
 * ep_return (double[N][3]);
 * hist (float[N][hist_stride], energy minus hist_ref, NaN = empty slot: every slot >= hist_len must be NaN);
 * t_win wb_win (double[N][weather_window_len]);  qtab (uint32[N][queue_stride][2]).
 * sdc_get_state only (diagnostics; refused where the batch has none, and by sdc_set_state always: they are derived from qtab / hist):
 * qcum_t (uint32[queue_stride][N], the time-major mirror of qtab's cum column), hist_t (uint32[hist_cap][N], the slot-major mirror of the
 * ring, raw keys). */
int sdc_get_state(sdc_handle* h, const char* field, void* host_buf, size_t bytes);
int sdc_set_state(sdc_handle* h, const char* field, const void* host_buf, size_t bytes);
/* a hash of the raw layouts a checkpoint holds (the record's and the header's dword offsets, the ring's stride): a checkpoint
 * is only meaningful to a library that returns the same value -- a re-laid-out record keeps its byte size */
uint32_t sdc_state_layout(void);
int sdc_hist_stride(const sdc_handle* h);
int sdc_queue_stride(const sdc_handle* h);

/* replaces: copy.deepcopy(env) of the reference's SustainDC (a plain Python object: what lookahead / MPC controllers, same-episode
 * policy comparisons and what-if studies branch an env with) for envs of one batch, on the device.  For each k, env dst[k] becomes an
 * exact copy of env src[k] as it stands after the work already queued on `stream`; the copy is ordered on `stream` like a step, and the
 * call does not synchronise the device.  The host waits in one case only: the index arrays are staged through two pinned buffers used
 * in turn, so a clone waits for the launch of the clone two calls back if that one has not finished yet.  src / dst: HOST arrays of n env indices.  Refused (nothing reaches the device): a null handle
 * or index array, n <= 0, an index outside [0, n_envs), a dst that appears twice, a dst that is also a src, no sdc_reset yet.
 * Copied: every per-env array the step, rollout, reset and verify kernels read -- the state record (assignment, day range and episode
 * counter included), the header (episode returns included), the history ring, the rank windows, the queue table, the weather windows,
 * the episode's feature rows, the queue table's and the ring's mirrors where the batch has them, the per-env config scalars (several
 * configs), the closed loop's copy of the latest observations (sdc_set_actor) -- and the caller's obs [N][3][26] / share_obs [N][29]
 * rows (device; either may be NULL), so that the buffer the next actions are chosen from is coherent.  A batch in lock-step before the
 * clone stays in lock-step when every src is at the same episode step: the next sdc_step / sdc_rollout runs the kernel it would have
 * run without the clone.
 * NOT copied: the env's global index (env_index_base + env), which keys its reset draws: dst finishes src's current episode exactly,
 * and from its next reset on it draws episodes of its own.
 * Deferred window re-centrings in flight: the copy clears the re-centring stamps of dst AND src (a result swept for src carries src's
 * index, so dst could never take it over, and the two would part in window placement; dst's own former request describes a state
 * that no longer exists) -- it does not move the launch counter as sdc_set_state does, which would drop the requests of every env of
 * the batch.  The windows concerned are re-requested by the step that needs them. */
int sdc_clone_envs(sdc_handle* h, const int32_t* src, const int32_t* dst, int n, float* obs, float* share_obs, void* stream);

/* replaces: copy.deepcopy(env) of the reference's SustainDC where the copy must outlive the batch or leave it -- rewinding an env
 * (lookahead / MPC: save at t, roll out candidate A, rewind, roll out candidate B), branching several policies from one state, moving
 * env states to an engine of another size, mapping or GPU.  An env's state goes to a row of a CALLER-OWNED device buffer and back.
 * A row is the env's complete state in a layout that depends on the state layout (sdc_state_layout) and on episode_steps alone --
 * never on n_envs, the mapping or the device: the state record (assignment, day range and episode counter included), the header
 * (episode returns included; its four deferred re-centring stamps are stored as zeros), the history ring, the rank windows, the
 * queue table, the weather windows, the episode's feature rows and the caller's obs [3][26] / share_obs [29] rows.  Not stored: the
 * queue table's and the ring's mirrors and the per-env config scalars -- derived data, rebuilt by the restore from the row.
 * sdc_snapshot_row_bytes: a row's size (a multiple of 256; ~145 KB at 672-step episodes), 0 for a null handle.
 * sdc_snapshot_envs: env envs[k] -> row k of rows [n][row_bytes] (device, 256-byte aligned); manifest [n][SDC_SNAPSHOT_MANIFEST] (HOST
 * int32) is filled at enqueue time from the host's mirrors.  READ-ONLY on the engine: the live env keeps its stamps and the launch
 * counter does not move, so taking snapshots does not change the run they are taken from.  envs may repeat; n <= n_envs.
 * sdc_restore_envs: env envs[k] becomes row rows_idx[k] of rows [n_rows][row_bytes] (this engine's or another's of the same state
 * layout, episode_steps, hist_cap, queue stride and weather window length); manifest [n_rows][SDC_SNAPSHOT_MANIFEST] as the snapshot
 * filled it.  One row may go to several envs; a dst must not appear twice.  The dst's stamps are cleared (as sdc_clone_envs does),
 * the feature rows go back into step-major order, the mirrors are rebuilt where this engine has them, the obs / share_obs rows go to
 * the caller's buffers and to the closed loop's copy.  The host's mirrors (episode step, feature rows, config, trace set) follow the
 * manifest: a restore that leaves every env of the batch at one episode step (a whole-batch rewind) keeps the specialised kernels,
 * one that leaves envs at different steps falls to the general kernel, as a masked reset does.
 * Both calls are ordered on `stream` like a step and do not synchronise the device (the index arrays are staged as sdc_clone_envs
 * stages its pairs); obs [N][3][26] / share_obs [N][29] are the caller's device buffers (required).  Refused (-2, nothing reaches the
 * device): a null handle or array, n <= 0 (n_rows <= 0), an env index outside [0, n_envs), a row index outside [0, n_rows), a repeated
 * dst, no sdc_reset yet, rows not 256-byte aligned, a manifest whose layout, episode_steps, hist_cap, queue stride or window length
 * differs from this engine's, a cfg_id / loc_id this engine does not have.
 * NOT part of an env's state: its global index (env_index_base + env) and the engine's seed.  A restored env finishes the saved episode
 * exactly; its later episodes are keyed on its own slot and the engine's seed -- so a rewind in place reproduces future episodes too. */
#define SDC_SNAPSHOT_MANIFEST 9
enum sdc_snapshot_manifest {
  SDC_SNAP_LAYOUT = 0,     /* sdc_state_layout() */
  SDC_SNAP_EPISODE_STEPS,
  SDC_SNAP_HIST_CAP,
  SDC_SNAP_QUEUE_STRIDE,   /* sdc_queue_stride() */
  SDC_SNAP_WINDOW_LEN,     /* sdc_weather_window_len() */
  SDC_SNAP_T_REL,          /* the env's episode step */
  SDC_SNAP_FEAT_OK,        /* 1: the row holds valid feature rows of the episode */
  SDC_SNAP_CFG_ID,
  SDC_SNAP_LOC_ID
};
size_t sdc_snapshot_row_bytes(const sdc_handle* h);
int sdc_snapshot_envs(sdc_handle* h, const int32_t* envs, int n, void* rows, int32_t* manifest, const float* obs,
                      const float* share_obs, void* stream);
int sdc_restore_envs(sdc_handle* h, const int32_t* rows_idx, const int32_t* envs, int n, const void* rows, int n_rows,
                     const int32_t* manifest, float* obs, float* share_obs, void* stream);

/* MARK AND REWIND: undo up to max_steps env-steps of an env in place -- the inner loop of lookahead / MPC ("mark at t, roll out candidate
 * A, rewind, roll out candidate B") at a fraction of a snapshot's cost.  A snapshot row is the env's complete state (~146 KB at
 * 672-step episodes); a MARK ROW holds only what max_steps steps INSIDE ONE EPISODE can change: the state record, the header (episode
 * returns included; its four deferred re-centring stamps stored as zeros), the four rank windows, the caller's obs [3][26] /
 * share_obs [29] rows, the max_steps history-ring slots the next appends go to (from the record's hist_len / hist_pos on: consecutive
 * slots, wrapping at hist_cap) and the max_steps queue-table entries from the env's episode step on (clipped at the table's end).
 * Not in the row because no step writes it: the rest of the ring and of the queue table, the weather windows, the episode's feature
 * rows, the per-env config scalars.  The mirrors of the queue table and the ring are derived: the rewind patches their rows of the
 * same slots from the row.
 * sdc_mark_row_bytes: roundup256(1964 + 12 * max_steps) -- 2 304 bytes for 16 steps, 2 816 for 64; 0 if max_steps is outside
 * [1, SDC_MARK_MAX_STEPS].  SDC_MARK_MAX_STEPS is 256: 2.7 days of a 15-minute episode, far beyond any lookahead horizon, and it keeps a
 * row (5 120 bytes) below 1/28 of a snapshot row.
 * sdc_mark_envs: env envs[k] -> row k of rows [n][row_bytes] (caller-owned device buffer, 256-byte aligned); manifest
 * [n][SDC_MARK_MANIFEST] (HOST int32) is filled at enqueue time.  envs == NULL: envs 0 .. n - 1 with n == n_envs (the whole batch: no
 * index staging).  READ-ONLY on the engine, as a snapshot is: the live env keeps its stamps and the launch counter does not move; a run
 * that takes marks is bit for bit the run without them.
 * sdc_rewind_envs: row k goes back into env envs[k] -- the SAME slot of the SAME engine it was taken from: record, header (stamps
 * cleared, as sdc_restore_envs and sdc_clone_envs do), rank windows, the ring slots and queue entries, the mirrors' rows of those where
 * the engine has mirrors, the caller's obs / share_obs rows and the closed loop's copy of obs.  The launch counter does not move.  The
 * host's mirror of the episode step follows the manifest: a whole-batch rewind of a lock-step batch stays on the kernel it was on, a
 * rewind of some envs leaves the batch out of lock-step, as a masked reset does.
 * ONE LIVE MARK PER ENV.  A row is only meaningful while everything it does not hold is unchanged; the library decides that from its
 * host mirrors, before anything reaches the device.  It keeps a serial per env: sdc_mark_envs gives the env a new one (its older mark is
 * dead from then on) and writes it to the manifest.  The serial is cleared -- every mark of the env dead -- by sdc_reset of the env
 * (masked or not), its auto-reset, sdc_set_state, and being a dst of sdc_clone_envs or sdc_restore_envs; being a clone src or a
 * snapshot source changes nothing.  A rewind leaves the mark alive: it may be repeated.  (Nested marks -- a stack per env for
 * depth-first search -- are out of scope: snapshots serve that.)
 * Both calls are ordered on `stream` like a step and do not synchronise the device; index arrays are staged as sdc_clone_envs stages its
 * pairs.  obs [N][3][26] / share_obs [N][29]: the caller's device buffers (required).  Refused (-2 and a message naming the reason,
 * nothing enqueued, all or nothing for the call): a null handle or array (other than envs), n <= 0, n > n_envs, envs == NULL with
 * n != n_envs, an index out of range or repeated, no sdc_reset yet, rows not 256-byte aligned, max_steps out of range; a rewind
 * additionally: a manifest of another state layout (sdc_state_layout) or engine, of another env than envs[k], a dead serial, an env
 * whose episode step is below the mark's, or MORE THAN max_steps STEPS TAKEN SINCE THE MARK -- slots beyond the row's reach have been
 * overwritten, so with that refusal the mark is dead for good.  This is the one side effect a refused call has: EVERY row of the call
 * whose mark has been overrun dies with it, also where the refusal names another row. */
#define SDC_MARK_MAX_STEPS 256
#define SDC_MARK_MANIFEST 7
enum sdc_mark_manifest {
  SDC_MARK_M_LAYOUT = 0,   /* sdc_state_layout() */
  SDC_MARK_M_ENGINE,       /* the engine's id (unique among the process's engines that have taken marks) */
  SDC_MARK_M_STEPS,        /* max_steps */
  SDC_MARK_M_ENV,          /* the env's index */
  SDC_MARK_M_SERIAL,       /* the env's serial at this mark (never 0) */
  SDC_MARK_M_T_REL,        /* the env's episode step at the mark */
  SDC_MARK_M_HIST_CAP
};
size_t sdc_mark_row_bytes(int max_steps);
int sdc_mark_envs(sdc_handle* h, const int32_t* envs, int n, int max_steps, void* rows, int32_t* manifest, const float* obs,
                  const float* share_obs, void* stream);
int sdc_rewind_envs(sdc_handle* h, const int32_t* envs, int n, const void* rows, const int32_t* manifest, float* obs, float* share_obs,
                    void* stream);

/* PLAN: score n_cand candidate action sequences of n_steps steps from the current state, pick the best one per env, and come back -- the
 * closing step of a shooting model-predictive controller that uses the simulator as its own model.  One call, ordered on `stream`, no
 * device synchronisation: the whole batch is marked (max_steps = n_steps) into a row buffer the handle owns; every candidate is rolled
 * out through sdc_rollout's own path (the same kernel choice) into an output block the handle owns -- never into a caller's buffer --,
 * scored by one launch of sdc_plan_score_kernel per rollout and rewound; sdc_plan_select_kernel then picks.  Afterwards the engine is
 * where a rewind leaves it: state rewound, the header's re-centring stamps cleared, the closed loop's copy of obs restored, the caller's
 * obs / share_obs rows (required, as for sdc_mark_envs / sdc_rewind_envs) holding what they held.  THE CALL USES UP THE ENVS' ONE LIVE
 * MARK: a mark the caller took earlier is dead afterwards.
 * actions [n_cand][n_steps][N][3] int32 (device); a slot on a built-in policy ignores its column, as in sdc_rollout.
 * objective (host; NULL: weights 1, 1, 1, gamma 1, no columns).  With g_0 = 1, g_k = g_{k-1} * gamma (an fp64 table built on the host),
 * r_k the step's three fp32 rewards and i_k its info row, all arithmetic in fp64 without fused multiply-adds, k = 0 .. n_steps - 1 in order:
 *   returns[c][n][a] = 0.0, then += g_k * r_k[a]                                                (may be NULL)
 *   s_k = (w[0] * r_k[0] + w[1] * r_k[1]) + w[2] * r_k[2], then for j = 0 .. n_cols - 1 in order += col_weight[j] * i_k[col[j]]
 *   score[c][n] = 0.0, then += g_k * s_k
 *   best[n] = the lowest c whose score is strictly greater than every earlier candidate's (candidate 0 unless a later one beats it with >)
 *   best_action[n][:] = actions[best[n]][0][n][:]
 * The output block is capped at 256 MiB (csrc/sdc_plan.hpp SDC_PLAN_SCRATCH_BYTES): where n_steps steps of outputs do not fit, a candidate is rolled out in chunks
 * of as many steps as fit (at least one) and the score kernel carries its sums across them -- a rollout of K steps equals K single
 * steps, so the results do not depend on the chunking.  debug_flags bit 14 (16384, TEST HOOK, read by this call alone): the block holds
 * two steps.
 * Refused (-2 and a message, nothing enqueued, the engine untouched): a null handle; n_cand < 1; n_steps outside
 * [1, SDC_MARK_MAX_STEPS]; n_steps >= sdc_steps_to_episode_end() with auto_reset (the reset would kill the mark), > without; no
 * sdc_reset yet; gamma outside (0, 1]; n_cols outside [0, SDC_PLAN_MAX_COLS] or a column outside [0, SDC_INFO_DIM); a null actions /
 * score / best / best_action / obs / share_obs; obs / share_obs rows that are not dword-aligned; verify mode (debug_flags bit 0), which
 * sdc_rollout refuses as well. */
#define SDC_PLAN_MAX_COLS 8
typedef struct {
  double reward_weight[3];   /* w_ls, w_dc, w_bat */
  double gamma;              /* discount per step, (0, 1] */
  int32_t n_cols;            /* 0..SDC_PLAN_MAX_COLS info columns in the objective */
  int32_t col[SDC_PLAN_MAX_COLS];     /* enum sdc_info_col, each in [0, SDC_INFO_DIM) */
  double col_weight[SDC_PLAN_MAX_COLS];
} sdc_plan_objective;
int sdc_plan(sdc_handle* h, int n_cand, int n_steps, const int32_t* actions, const sdc_plan_objective* objective, double* returns,
             double* score, int32_t* best, int32_t* best_action, float* obs, float* share_obs, void* stream);

/* PLAN TERMS: what a linear objective cannot say -- operating limits ("stay below 27 degrees", "SOC never under 0.2": a hinge on an info
 * column, charged every step) and a terminal term (weights on the info row the horizon's LAST step leaves: queue length, overdue tasks,
 * the battery's charge -- what a finite horizon otherwise defers for free).  The terms are host state of the handle: sdc_set_plan_terms
 * copies them, and every later sdc_plan, sdc_plan_cem and sdc_plan_cem_groups call scores with them until they are cleared (terms NULL,
 * or both counts 0).  While terms are set those calls score a rollout with sdc_plan_score_terms_kernel (csrc/sdc_plan_terms.hip) in
 * place of sdc_plan_score_kernel; with none set the launch is sdc_plan_score_kernel, as before the terms existed.  Neither call touches
 * the device.  sdc_get_plan_terms copies out what is set (cleared: every field 0).
 * The arithmetic, in sdc_plan's words (fp64, no fused multiply-adds, steps k = 0 .. n_steps - 1 in order; s_k as sdc_plan defines it:
 * the rewards first, then the objective's own columns), with i_k the step's info row:
 *   for j = 0 .. n_limits - 1 in order, x = (double) i_k[limit_col[j]]:
 *     d = limit_side[j] > 0 ? x - limit_bound[j] : limit_bound[j] - x
 *     e = d > 0.0 ? d : 0.0                (a compare and a select: a NaN x gives e = 0)
 *     s_k = s_k - limit_weight[j] * e
 *   score += g_k * s_k                     (as in sdc_plan)
 *   after the horizon's last step k = n_steps - 1 only:
 *     t = 0.0, then for j = 0 .. n_terminal - 1 in order += terminal_weight[j] * (double) i_k[terminal_col[j]]
 *     score += (g_{n_steps-1} * gamma) * t     (the discount one fp64 multiply on the host)
 * `returns` do not see the terms.  Nothing downstream changes: sdc_plan's selection rule and the CEM calls' ranking, elites and refit
 * are what they were and see these scores.  A horizon rolled out in chunks applies the terminal term once, in its last chunk.
 * Refused (-2 and a message; the terms set before stay in force): a null handle; n_limits outside [0, SDC_PLAN_MAX_LIMITS], n_terminal
 * outside [0, SDC_PLAN_MAX_TERMINAL]; a limit_col or terminal_col outside [0, SDC_INFO_DIM); a limit_side other than +1 / -1; a
 * limit_bound, limit_weight or terminal_weight that is not finite; a negative limit_weight.  sdc_get_plan_terms: a null handle or out. */
#define SDC_PLAN_MAX_LIMITS 8
#define SDC_PLAN_MAX_TERMINAL 8
typedef struct {
  int32_t n_limits;                                /* 0..SDC_PLAN_MAX_LIMITS */
  int32_t limit_col[SDC_PLAN_MAX_LIMITS];          /* enum sdc_info_col */
  int32_t limit_side[SDC_PLAN_MAX_LIMITS];         /* +1: upper bound, -1: lower bound */
  double limit_bound[SDC_PLAN_MAX_LIMITS];         /* finite */
  double limit_weight[SDC_PLAN_MAX_LIMITS];        /* finite, >= 0: penalty per unit of excess per step */
  int32_t n_terminal;                              /* 0..SDC_PLAN_MAX_TERMINAL */
  int32_t terminal_col[SDC_PLAN_MAX_TERMINAL];
  double terminal_weight[SDC_PLAN_MAX_TERMINAL];   /* finite */
} sdc_plan_terms;
int sdc_set_plan_terms(sdc_handle* h, const sdc_plan_terms* terms);
int sdc_get_plan_terms(const sdc_handle* h, sdc_plan_terms* out);

/* THE CRITIC.  replaces: the V critic's forward pass (harl/models/value_function_models/v_net.py VNet over harl/models/base/mlp.py
 * MLPBase, hidden_sizes [64, 64], no recurrence) and harl/common/valuenorm.py ValueNorm.denormalize, over rows of share_obs:
 *     LayerNorm(29) -> Linear(29, 64) -> act -> LayerNorm(64) -> Linear(64, 64) -> act -> LayerNorm(64) -> Linear(64, 1);  v * scale + shift
 * fp32 throughout (LayerNorm: biased variance, eps 1e-5), the two hidden layers on fp32-input matrix instructions, 16 rows per wavefront
 * (csrc/sdc_rowmlp.hpp).  sdc_critic_params is torch's layout ([out][in], row-major), as sdc_actor_params is; flags bit 0: the feature
 * LayerNorm is on (off: ln0_g / ln0_b are not used, but must be finite), bits 1-2: the activation, 0 tanh, 1 relu.  scale and shift fold a
 * ValueNorm (sqrt of its debiased variance, its debiased mean); 1 and 0 without one.
 * sdc_set_critic packs the parameters into the kernels' layout and copies them to the handle's device (host pointer; it waits for the
 * device first: a launch in flight may still read the critic set before).  Refused (-2 and a message; the critic set before stays in
 * force): a null handle or params; an entry that is not finite; scale <= 0; flag bits above bit 2 or an activation code above 1.
 * sdc_critic_values: values[r] = the critic's value of share_obs row r, r < n_rows -- rows [n_rows][29] fp32, 116 bytes apart, device
 * memory, dword-aligned; one launch of sdc_critic_values_kernel on `stream`, no synchronisation; a row's value does not depend on which
 * other rows the call holds or on their order.  Refused: a null handle; no critic set; a null or not dword-aligned share_obs or values;
 * n_rows < 1.  sdc_last_step_kernel names the kernel afterwards.
 * THE PLAN CRITIC: the critic as the planners' terminal value -- MPC with a learned value at the horizon's end.  The weight is host state
 * of the handle, next to the plan terms: sdc_set_plan_critic stores it, and while it is not 0 every later sdc_plan, sdc_plan_cem and
 * sdc_plan_cem_groups call (and through them sdc_rollout_cem_stats and sdc_rollout_cem_groups_stats, whose predicted score then includes
 * the term) launches, per candidate, one sdc_critic_terminal_kernel behind the score launch of the chunk that holds the horizon's last
 * step and in front of the rewind.  With s_n the share_obs row env n (a replica is an env row) has after step n_steps - 1 of the
 * candidate's rollout and done_n that step's done flag:
 *     V_n = the value sdc_critic_values gives for s_n, bit for bit
 *     score[n] = score[n] + ((g_{n_steps-1} * gamma) * weight) * (done_n ? 0.0 : (double) V_n)
 * fp64, no fused multiply-add; the two factors in front are multiplied on the host, in that order.  An episode that ends with the horizon
 * has no value behind it: the term is 0 there.  `returns` do not see the term; the plan terms, the selection rule and the CEM calls'
 * ranking, elites and refit are what they were and see these scores.  With weight 0 (the default) nothing is launched and every result
 * is bit for bit what it is without a critic.  sdc_last_step_kernel names sdc_critic_terminal_kernel after a plan call that launched it
 * (the rewind behind it launches no step kernel).
 * Refused: a null handle (or out); a weight that is not finite; a weight other than 0 while no critic is set. */
typedef struct {
  float ln0_g[29], ln0_b[29];                        /* base.feature_norm */
  float w1[64 * 29], b1[64], ln1_g[64], ln1_b[64];   /* base.mlp.fc.0, fc.2 */
  float w2[64 * 64], b2[64], ln2_g[64], ln2_b[64];   /* base.mlp.fc.3, fc.5 */
  float w3[64], b3;                                  /* v_out */
  float scale, shift;                                /* > 0, finite */
  int32_t flags;
} sdc_critic_params;
int sdc_set_critic(sdc_handle* h, const sdc_critic_params* p);
int sdc_critic_values(sdc_handle* h, const float* share_obs, long long n_rows, float* values, void* stream);
int sdc_set_plan_critic(sdc_handle* h, double weight);
int sdc_get_plan_critic(const sdc_handle* h, double* weight);

/* THE ON-POLICY BATCH.  replaces: what the reference's on-policy runners build on the host, in NumPy, from a collected rollout
 * (harl/runners/on_policy_base_runner.py insert / compute, harl/common/buffers/on_policy_critic_buffer_ep.py compute_returns -- a Python
 * loop of episode_length iterations --, harl/runners/on_policy_ha_runner.py and harl/algorithms/actors/happo.py for the advantages and
 * their normalisation, the actors' evaluate_actions for the log-probabilities).  Both calls are pure functions of their arrays, all
 * device memory, N = the handle's n_envs, T = n_steps: they read no env state and move nothing in the engine; each is ordered on
 * `stream` with no synchronisation (sdc_gae's [N][2] fp64 partial sums are a buffer of the handle's, allocated on first use).
 * sdc_gae: the backward pass of compute_returns for the EP state type, one launch of sdc_gae_kernel (one lane per env) and, when
 * `moments` is given, one single-workgroup launch of sdc_adv_moments_kernel behind it (csrc/sdc_onpolicy.hip).
 *   rew [T][N][3] fp32, of which column reward_agent is read (the reference feeds rewards[:, 0]);  done [T][N] uint8;
 *   first_done [N] uint8 or NULL: the done flags of the step before the batch's first (NULL: none was done);
 *   values [T+1][N] fp32: the critic's DENORMALISED values of the T+1 share_obs rows, as sdc_critic_values gives them with a ValueNorm
 *   folded in; row T is the bootstrap.
 * Everything is fp32, no fused multiply-add, in the reference's order of operations:
 *     g = (float)gamma;  c = (float)(gamma * gae_lambda)        // the product in double, rounded once: NumPy's weak Python scalars
 *   for t = T-1 .. 0, per env n:
 *     m = done[t][n] ? 0.0f : 1.0f                              // the reference's masks[t + 1]
 *     use_gae:   delta = (r + (g * V[t+1]) * m) - V[t];   gae = delta + (c * m) * gae;   returns[t] = gae + V[t]        (gae starts at 0)
 *     otherwise: ret = (ret * g) * m + r   (ret starts at V[T]);   returns[t] = ret
 *     advantages[t] = returns[t] - V[t]
 * (use_proper_time_limits makes no difference: the reference sets bad_masks nowhere, they are all ones.)
 *   returns [T][N], advantages [T][N]: written once per env and step;
 *   masks [T+1][N] fp32: masks[0][n] = first_done && first_done[n] ? 0 : 1, masks[t+1][n] = m;
 *   value_preds [T+1][N] fp32 or NULL: (V - shift) / scale in fp32 with the scale and shift of the critic set on the handle (the
 *     ValueNorm folded into it): the normalised predictions the reference's clipped value loss keeps in its buffer, RECOMPUTED from the
 *     denormalised values -- within a few ulp of, not the bits of, the network's raw output;
 *   moments [2] fp64, 16-byte aligned, or NULL (no second launch): the mean of the T N advantages and their population standard
 *     deviation sqrt(max(E[x^2] - mean^2, 0)), E[x^2] = (sum of squares) / (T N), mean = sum / (T N) -- the reference's nanmean / nanstd
 *     where all agents finish together and active_masks is all ones.  Per env the sum of (double)a and of (double)a * (double)a over
 *     its advantages in the walk's order t = T-1 .. 0; then with B = 256 partial pair l the sum over envs l, l + B, l + 2 B, ... in that
 *     order, then partial i += partial i + half for half = B/2 .. 1: a fixed order, no atomics, the same bits on every run.
 * Refused (-2 and a message, nothing enqueued): a null handle; n_steps < 1; a null rew, done, values, returns, advantages or masks; rew,
 * values, returns, advantages, masks or value_preds not dword-aligned; moments not 16-byte aligned; reward_agent outside 0 .. 2; use_gae
 * outside {0, 1}; gamma or gae_lambda not finite or outside [0, 1]; value_preds given while no critic is set.
 * sdc_action_log_probs: one launch of sdc_action_logp_kernel, one lane per (step, env, agent).  With j = actions[t][n][a] (an action
 * outside 0 .. 2 is read as 2) and l0, l1, l2 = logits[t][n][a][0..2], in sdc_rollout_actor_stats' arithmetic, word for word:
 *     m = max(l0, l1, l2) in fp32;   z_i = (double)l_i - (double)m;   e_i = exp(z_i);   s = (e0 + e1) + e2;   lse = log(s)
 *     lp_i = z_i - lse;   p_i = e_i / s
 *     log_probs[t][n][a] = (float)lp_j;   entropy[t][n][a] = (float)(-((p0 * lp0 + p1 * lp1) + p2 * lp2))
 * fp64 without fused multiply-adds, each result rounded once to fp32.  actions [T][N][3] int32, logits [T][N][3][3] fp32, log_probs and
 * entropy [T][N][3] fp32; entropy may be NULL.  Refused: a null handle; n_steps < 1; a null actions, logits or log_probs; an array that
 * is not dword-aligned. */
int sdc_gae(sdc_handle* h, int n_steps, const float* rew, int reward_agent, const uint8_t* done, const uint8_t* first_done,
            const float* values, double gamma, double gae_lambda, int use_gae, float* returns, float* advantages, float* masks,
            float* value_preds, double* moments, void* stream);
int sdc_action_log_probs(sdc_handle* h, int n_steps, const int32_t* actions, const float* logits, float* log_probs, float* entropy,
                         void* stream);

/* EVALUATE THE ACTORS ON STORED ROWS.  replaces: the forward pass of the reference's evaluate_actions over a stored buffer
 * (harl/algorithms/actors/on_policy_base.py evaluate_actions -> StochasticPolicy.evaluate_actions), which harl/runners/on_policy_ha_runner.py
 * runs over the whole buffer before and after every agent's update for the HAPPO factor, and the terms harl/algorithms/actors/happo.py and
 * mappo.py build from its log-probabilities (imp_weights, the clipped surrogate, the entropy).  No gradient: the backward pass is
 * sdc_actor_backward (THE ACTORS' GRADIENT below), the critic's value loss is THE CRITIC'S GRADIENT's; the optimiser is THE OPTIMISER STEP, shuffled mini-batches are TRAIN ON THE DEVICE.  Both calls are pure functions of their arrays, all device memory: they read no env
 * state and move nothing in the engine; each is ordered on `stream` with no synchronisation.
 * sdc_actor_evaluate: the logits of agent_slot's network -- the one last given to sdc_set_actor for that slot, the network stated at
 * sdc_set_actor, fp32, the hidden layers on fp32-input matrix instructions, 16 rows per wavefront (csrc/sdc_rowmlp.hpp) -- for n_rows
 * rows of observations, ONE launch of sdc_actor_eval_kernel.  Row r is the 26 floats at obs + r * row_stride (floats; row_stride 26: a
 * dense per-agent buffer; 78 with obs advanced by 26 * agent: the agent's rows of an [..][3][26] array as sdc_rollout_actor fills it); its
 * three logits go to logits + r * logits_stride (logits_stride 3: dense; 9 with logits advanced by 3 * agent: the agent's column of a
 * [T][N][3][3] array, on which sdc_action_log_probs runs unchanged).  Nothing else is written: the floats between two rows' logits keep
 * their values.  A row's logits depend on that row and the parameters alone -- not on its position, the strides, n_rows or the rows next
 * to it -- to the bit; against the closed loop's logits of the same row (sdc_rollout_actor sums in another order) they agree to fp32
 * rounding, not to the bit.
 * Refused (-2 and a message, nothing enqueued): a null handle; agent_slot outside 0 .. 2; no actor set for that slot; n_rows < 1; a null
 * obs or logits; obs or logits not dword-aligned; row_stride < 26; logits_stride < 3.
 * sdc_ppo_terms: per element i = t N + n < T N (N = the handle's n_envs, T = n_steps), with j = 3 i + agent, in fp64 with no fused
 * multiply-add, each stored value rounded once to fp32:
 *     lr = (double)new_log_probs[j] - (double)old_log_probs[j]           // exact
 *     r  = exp(lr);                        ratio[i] = (float)r           // the reference's imp_weights
 *     A  = (double)advantages[i];          F = factor ? (double)factor[i] : 1.0
 *     s1 = r * A;    rc = r < lo ? lo : r;   rc = rc > hi ? hi : rc;    s2 = rc * A      // lo = 1 - clip_param, hi = 1 + clip_param, in double
 *     surr[i] = (float)(F * (s2 < s1 ? s2 : s1))
 *     factor_out[i] = (factor ? factor[i] : 1.0f) * ratio[i]             // ONE fp32 product of the stored values: the runner's
 *                                                                        // factor * exp(new - old); factor_out may be the array `factor`
 *     clipped_i = r < lo || r > hi
 * new_log_probs, old_log_probs, entropy [T][N][3] fp32, of which column `agent` alone is read (the other columns may hold anything);
 * advantages, factor, ratio, surr, factor_out [T][N] fp32; entropy, factor, surr, factor_out and stats may be NULL (factor NULL: 1, MAPPO).
 * stats [8] fp64 or NULL: fp64 statistics of the STORED fp32 values, so that a host redoes them bit for bit from the call's outputs:
 *     0 sum of (double)surr[i] (whether or not surr is stored)    1 sum of (double)ratio[i]    2 sum of lr    3 sum of (double)entropy[j]
 *     (0 without entropy)    4 number of clipped elements    5 min of (double)ratio[i]    6 max of (double)ratio[i]    7 (double)(T N)
 * in a fixed order, no atomics, the same bits on every run -- two launches, sdc_ppo_terms_kernel and sdc_ppo_stats_kernel:
 *   stage 1: B = min(ceil(T N / 256), 1024) workgroups of 256 lanes.  Lane l of workgroup b starts from (0, 0, 0, 0, 0, +inf, -inf) and
 *     folds the elements i = b * 256 + l + k * 256 * B, k = 0, 1, ... (i < T N) in that order: sums s = s + x, minimum m = x < m ? x : m,
 *     maximum m = x > m ? x : m.  Then for half = 128, 64, .. 1: lane l < half takes lane l + half (sums a + b, minimum b < a ? b : a,
 *     maximum b > a ? b : a); lane 0's is partial b.
 *   stage 2: one workgroup of 256 lanes.  Lane l starts as above and takes partials l, l + 256, ... (< B) in that order, then the same
 *     halving; lane 0's values are stats[0..6], and stats[7] = (double)(T N).
 * With stats NULL neither reduction runs (one launch).  The partials are a buffer of the handle's, allocated on first use.
 * Refused: a null handle; n_steps < 1; agent outside 0 .. 2; a null new_log_probs, old_log_probs, advantages or ratio; a float array not
 * dword-aligned; stats not 8-byte aligned; clip_param not finite or outside [0, 1). */
int sdc_actor_evaluate(sdc_handle* h, int agent_slot, const float* obs, long long row_stride, long long n_rows, float* logits,
                       long long logits_stride, void* stream);
int sdc_ppo_terms(sdc_handle* h, int n_steps, int agent, const float* new_log_probs, const float* old_log_probs, const float* entropy,
                  const float* advantages, const float* factor, double clip_param, float* ratio, float* surr, float* factor_out,
                  double* stats, void* stream);

/* THE ACTORS' GRADIENT.  replaces: loss.backward() of the reference's actor update (harl/algorithms/actors/happo.py update:
 * policy_loss - entropy_coef * dist_entropy, differentiated by autograd through StochasticPolicy.evaluate_actions) -- the gradient with
 * respect to every parameter of one agent's network, on fp32-input matrix instructions, in a fixed summation order.  NOT here: the
 * optimiser step (sdc_actor_adam_step, THE OPTIMISER STEP below; or a caller steps an optimiser over the SDC_ACTOR_N_PARAMS values and calls sdc_set_actor)
 * and minibatch shuffling (sdc_permutation and sdc_gather_rows, TRAIN ON THE DEVICE below: the rows are made dense, then these calls run on them);
 * the critic's value loss and its gradient are THE CRITIC'S GRADIENT below.  Both calls are pure functions of their arrays, all device memory: they read no
 * env state and move nothing in the engine; each is ordered on `stream` with no synchronisation.
 * sdc_ppo_dlogp: the loss's derivative per stored log-probability, ONE launch of sdc_ppo_dlogp_kernel.  Per element i = t N + n < T N
 * with j = 3 i + agent, in fp64 with no fused multiply-add, in sdc_ppo_terms' words (lo = 1 - clip_param, hi = 1 + clip_param):
 *     lr = (double)new_log_probs[j] - (double)old_log_probs[j];   r = exp(lr);   A = (double)advantages[i];   F = factor ? (double)factor[i] : 1.0
 *     s1 = r * A;   rc = r < lo ? lo : r;   rc = rc > hi ? hi : rc;   s2 = rc * A;   clipped = r < lo || r > hi
 *     open = !clipped || s1 < s2
 *     dlogp[i] = (float)(open ? -(((scale * F) * A) * r) : 0.0)
 * which is d(-scale * sum_i F min(s1, s2)) / d new_log_probs[j] as torch differentiates it (torch.min halves a tie, clamp passes the
 * gradient on its closed interval: together the rule `open`).  scale: a finite double; 1 / (T N) is the reference's mean with every
 * active mask one.  Refused: what sdc_ppo_terms refuses about the arguments they share, a null or misaligned dlogp, a scale not finite.
 * sdc_actor_backward: with logp_r(a) and H_r the log-probability and the entropy of row r's categorical distribution under the network
 * last given to sdc_set_actor for agent_slot, the gradient of
 *     L = sum_r dlogp[r] * logp_r(actions_r) + dent * sum_r H_r
 * with respect to the float members of sdc_actor_params in declaration order (ln0_gamma .. b3, torch's [out][in] layout), fp32
 * [SDC_ACTOR_N_PARAMS] in `grads`.  Row r is the 26 floats at obs + r * row_stride (as sdc_actor_evaluate's), its action
 * actions[r * action_stride] (1: dense; 3 with actions advanced by agent: the agent's column of [T][N][3]) -- a value outside 0 .. 2 is
 * an all-zero one-hot: it enters arithmetic only, never an address --, its coefficient dlogp[r], dense; dent = dL/dH_r is the same for
 * every row (the reference: -entropy_coef / n_rows).  The backward is the textbook one over the call's own forward
 * (csrc/sdc_actor_grad.hpp, fp32): with p = softmax(logits)
 *     dlogit_c = dlogp[r] * (1[c == a_r] - p_c) - dent * (p_c * (log p_c + H_r))
 *     Linear:     dW += dz x^T, db += dz, dx = W^T dz
 *     LayerNorm:  dgain += dy * n, dbias += dy, dn = dy * gain, dx = rs * (dn - mean(dn) - n * mean(dn * n)), n and rs the forward's
 *                 (the forward's clamp of the variance at 0 is not differentiated)
 *     tanh' = 1 - h * h from the forward's own h;  relu' = [z > 0]
 * The feature LayerNorm's gain and bias receive gradients when use_feature_normalization is on and exact zeros when it is off; nothing
 * is propagated to obs.  Doubling dlogp and dent doubles every gradient exactly; all-zero coefficients give all-zero gradients.
 * THE ORDER OF EVERY SUM IS FIXED -- no atomics, the same call gives the same bits on every run: B = min(ceil(n_rows / 64),
 * SDC_ACTOR_GRAD_MAX_BLOCKS) workgroups (a function of n_rows alone) each write one fp32 partial [SDC_ACTOR_N_PARAMS] into a buffer
 * of the handle's, allocated on first use (sdc_actor_grad_kernel; within it: csrc/sdc_actor_grad.hpp); sdc_actor_grad_reduce_kernel
 * adds a parameter's B partials in workgroup order in fp64 and rounds once to fp32.
 * grad_sq [1] fp64 or NULL: the sum of squares of the STORED fp32 grads, so that a host redoes it bit for bit
 * (sdc_actor_grad_sq_kernel, one workgroup of 256 lanes): lane l starts from 0 and adds (double)grads[j] * (double)grads[j] for
 * j = l, l + 256, ... < SDC_ACTOR_N_PARAMS in that order; then for half = 128, 64, .. 1 lane l < half adds lane l + half; lane 0's sum.
 * Refused (-2 and a message, nothing enqueued): a null handle; agent_slot outside 0 .. 2; no actor set for that slot; n_rows < 1; a
 * null obs, actions, dlogp or grads; one of them not dword-aligned; grad_sq not 8-byte aligned; row_stride < 26; action_stride < 1;
 * dent not finite. */
#define SDC_ACTOR_N_PARAMS 6391
#define SDC_ACTOR_GRAD_MAX_BLOCKS 256
int sdc_ppo_dlogp(sdc_handle* h, int n_steps, int agent, const float* new_log_probs, const float* old_log_probs, const float* advantages,
                  const float* factor, double clip_param, double scale, float* dlogp, void* stream);
int sdc_actor_backward(sdc_handle* h, int agent_slot, const float* obs, long long row_stride, long long n_rows, const int32_t* actions,
                       long long action_stride, const float* dlogp, double dent, float* grads, double* grad_sq, void* stream);

/* THE CRITIC'S GRADIENT.  replaces: the critic's half of an on-policy update (harl/algorithms/critics/v_critic.py cal_value_loss and
 * update's loss.backward(), harl/utils/models_tools.py huber_loss / mse_loss, harl/common/valuenorm.py normalize) -- the network's own
 * output over stored share_obs rows, the clipped Huber / MSE value loss with its derivative per row, and the gradient with respect to
 * every parameter of the critic.  NOT here: the optimiser step (sdc_critic_adam_step, THE OPTIMISER STEP below, or a caller's own optimiser and sdc_set_critic),
 * ValueNorm's running update and minibatch shuffling (sdc_value_norm_update, sdc_permutation and sdc_gather_rows, TRAIN ON THE DEVICE
 * below: the normaliser is updated first, as the reference does it, and sdc_value_loss_normed reads the new statistics).  All three
 * calls are pure functions of their arrays, all device memory: they read no env state and move nothing in the engine; each is ordered
 * on `stream` with no synchronisation; no atomics: the same call gives the same bits on every run.
 * sdc_critic_evaluate: raw_values[r] = u_r, the network's own output for share_obs row r BEFORE `* scale + shift` -- what the
 * reference's critic(cent_obs) returns under a ValueNorm --, rows [n_rows][29] dense as sdc_critic_values'; ONE launch of
 * sdc_critic_raw_kernel.  sdc_critic_values of the same row is (u_r * scale) + shift in fp32 with no fused multiply-add, bit for bit.
 * Refused: what sdc_critic_values refuses.
 * sdc_value_loss: per element i < n, with u, vp, ret = raw_values[i], value_preds[i], returns[i] widened to fp64, clip = clip_param,
 * delta = huber_delta, in fp64 with no fused multiply-add, each stored result rounded once to fp32:
 *     t   = (ret - target_shift) / target_scale            // ValueNorm.normalize; 1 and 0 without one
 *     d   = u - vp;  dc = d < -clip ? -clip : (d > clip ? clip : d);  uc = vp + dc
 *     eo  = t - u;   ec = t - uc
 *     l(e)  = huber ? (|e| <= delta ? (e * e) / 2 : delta * (|e| - delta / 2)) : (e * e) / 2
 *     l'(e) = huber ? (|e| <= delta ? e : (e > 0 ? delta : -delta)) : e
 *     go  = -l'(eo);   gc = (-clip <= d && d <= clip) ? -l'(ec) : 0
 *     clipped loss on:   L = l(eo) > l(ec) ? l(eo) : l(ec);
 *                        g = l(eo) > l(ec) ? go : (l(eo) < l(ec) ? gc : 0.5 * go + 0.5 * gc)
 *     clipped loss off:  L = l(eo);  g = go
 *     loss[i] = (float)L;   dvalue[i] = (float)(coef * g)
 * which is d(coef * sum_i L_i) / d u_i as torch differentiates the reference (clamp passes the gradient on its closed interval, the
 * binary torch.max halves a tie, the Huber masks are constants).  flags bit 0: Huber loss (off: (e * e) / 2), bit 1: clipped value
 * loss.  coef: a finite double; the reference's is value_loss_coef / n.  loss and stats may be NULL.
 * stats [8] fp64 or NULL: 0 sum of (double)loss[i] (whether or not loss is stored)   1 sum of u   2 sum of eo   3 sum of eo * eo
 *     4 number of elements with l(ec) > l(eo)   5 min of eo   6 max of eo   7 (double)n
 * in sdc_ppo_terms' fixed two-stage order, word for word (B = min(ceil(n / 256), 1024) workgroups of 256 lanes, the same folding and
 * halving; stage 2 IS sdc_ppo_stats_kernel): two launches, sdc_value_loss_kernel and sdc_ppo_stats_kernel; with stats NULL one.  The
 * partials are a buffer of the handle's, allocated on first use.  It reads nothing from the handle but its device.
 * Refused (-2 and a message, nothing enqueued): a null handle; n < 1; a null raw_values, value_preds, returns or dvalue; a float array
 * not dword-aligned; stats not 8-byte aligned; target_scale not finite or <= 0; target_shift not finite; clip_param not finite or < 0;
 * flag bits above bit 1; huber_delta not finite or <= 0 while bit 0 is set; coef not finite.
 * sdc_critic_backward: with u_r the raw output of the critic last given to sdc_set_critic for share_obs row r, the gradient of
 *     L = sum_r dvalue[r] * u_r
 * with respect to the float members of sdc_critic_params from ln0_g to b3 in declaration order (torch's [out][in] layout), fp32
 * [SDC_CRITIC_N_PARAMS] in `grads`; scale and shift are no parameters and get no gradient; nothing is propagated to share_obs.  The
 * backward is THE ACTORS' GRADIENT's (Linear, LayerNorm, tanh' / relu' as stated there) over the call's own forward
 * (csrc/sdc_critic_grad.hpp, fp32); the head has one output: dy2 = w3 * dvalue[r], db3 = sum_r dvalue[r], and with S = sum_r dvalue[r]
 * * n2_r (n2: the second hidden LayerNorm's normalised values) dgain2 = w3 * S, dbeta2 = w3 * db3, dW3 = gain2 * S + beta2 * db3 -- per
 * wavefront of a workgroup, then summed as everything else.  The feature LayerNorm's gain and bias receive gradients when flags bit 0
 * is on and exact zeros when it is off.  Doubling dvalue doubles every gradient exactly; all-zero coefficients give all-zero gradients.
 * THE ORDER OF EVERY SUM IS FIXED as sdc_actor_backward's: B = min(ceil(n_rows / 64), SDC_CRITIC_GRAD_MAX_BLOCKS) workgroups (a
 * function of n_rows alone) each write one fp32 partial [SDC_CRITIC_N_PARAMS] into a buffer of the handle's, allocated on first use
 * (sdc_critic_grad_tanh_kernel / sdc_critic_grad_relu_kernel); sdc_critic_grad_reduce_kernel adds a parameter's B partials in
 * workgroup order in fp64 and rounds once to fp32.  grad_sq [1] fp64 or NULL: the sum of squares of the STORED fp32 grads in the order
 * sdc_actor_backward documents, over SDC_CRITIC_N_PARAMS values (sdc_critic_grad_sq_kernel).
 * Refused (-2 and a message, nothing enqueued): a null handle; no critic set; n_rows < 1; a null share_obs, dvalue or grads; one of
 * them not dword-aligned; grad_sq not 8-byte aligned. */
#define SDC_CRITIC_N_PARAMS 6459
#define SDC_CRITIC_GRAD_MAX_BLOCKS 256
int sdc_critic_evaluate(sdc_handle* h, const float* share_obs, long long n_rows, float* raw_values, void* stream);
int sdc_value_loss(sdc_handle* h, long long n, const float* raw_values, const float* value_preds, const float* returns, double target_scale,
                   double target_shift, double clip_param, double huber_delta, int flags, double coef, float* loss, float* dvalue,
                   double* stats, void* stream);
int sdc_critic_backward(sdc_handle* h, const float* share_obs, long long n_rows, const float* dvalue, float* grads, double* grad_sq,
                        void* stream);

/* THE OPTIMISER STEP.  replaces: the last link of an on-policy update (torch.optim.Adam.step() behind nn.utils.clip_grad_norm_ in
 * harl/algorithms/actors/happo.py and critics/v_critic.py update) and the round trip through the host that followed it.  From the
 * first sdc_set_actor / sdc_set_critic on the handle keeps, per actor slot and for the critic, on the device: a master copy
 * params[SDC_*_N_PARAMS] fp32 in the order of `grads`, Adam's moments m[] and v[] fp32 of that length, and a state block
 * (sdc_optim_state).  sdc_set_actor / sdc_set_critic do what they always did and also fill the master copy, zero the moments and
 * reset the state block to {0, 1.0, 1.0, 0}: a new network gets a new optimiser.
 * sdc_actor_adam_step / sdc_critic_adam_step: one Adam step with gradient-norm clipping over `grads` ([SDC_*_N_PARAMS] fp32 device
 * memory, as sdc_*_backward wrote it, UNCLIPPED), then every packed copy the kernels read (an actor's three, the critic's two) is
 * rewritten from the master copy.  Ordered on `stream`: no synchronisation, no device memory read by the host, no atomics, TWO
 * launches (sdc_adam_update_kernel on one workgroup, sdc_adam_gather_kernel on twenty; csrc/sdc_optim.hip).  Launches in front of it on the same stream see
 * the old weights, launches behind it the new ones; ORDERING AGAINST OTHER STREAMS IS THE CALLER'S (a rollout on another stream may
 * read a packed copy while it is rewritten).  The arithmetic (csrc/sdc_optim.hpp holds it once, for the device and for a host
 * compiler), g = grads as given:
 *   1. S = the fp64 sum of squares of g in exactly sdc_actor_backward's grad_sq order (256 lanes, strided, tree from 128 down);
 *      sqrt(S) is the norm of that call's grad_sq bit for bit.  grad_norm [1] fp64 device memory or NULL receives sqrt(S).
 *   2. S not finite (a NaN or infinity somewhere in g): skipped += 1 and NOTHING else changes -- parameters, moments, step, the
 *      powers and every packed copy keep their bits.
 *   3. c = min(1.0, max_grad_norm / (sqrt(S) + 1e-6)) in fp64, rounded once to fp32 (torch's clip_grad_norm_ rule).
 *   4. step += 1; beta1_pow *= beta1; beta2_pow *= beta2 in fp64; step_size = (float)(lr / (1 - beta1_pow));
 *      rsq = (float)sqrt(1 - beta2_pow); beta2, 1 - beta1, 1 - beta2 (formed in fp64), eps and weight_decay each rounded once to fp32.
 *   5. per element, fp32, correctly rounded division and square root, no fused multiply-add, one rounding per operation, in the form
 *      of torch/optim/adam.py _single_tensor_adam:
 *          g = g * c;   if (weight_decay != 0) g = g + weight_decay * p
 *          m = m + (1 - beta1) * (g - m)                       (lerp_, the form of weights below 0.5, unfused)
 *          v = v * beta2;   v = v + ((1 - beta2) * g) * g      (mul_ / addcmul_)
 *          denom = sqrt(v) / rsq + eps;   p = p - step_size * (m / denom)
 *      Where torch's kernels differ among themselves this is the CPU kernels' order of operations without their fused multiply-adds:
 *      a division by rsq (not a multiplication by its reciprocal), value * t1 * t2 left to right in addcmul, value * (t1 / t2) in
 *      addcdiv.
 *   6. with the network's feature LayerNorm off its ln0 entries (the first 52 / 58 values) are not touched, not even by weight decay.
 * Refused (-2 and a message, nothing enqueued): a null handle; agent_slot outside 0 .. 2; no actor / critic set; null or not
 * dword-aligned grads; grad_norm not 8-byte aligned; a null sdc_adam; lr, eps or weight_decay not finite or negative; a beta outside
 * [0, 1); max_grad_norm NaN or not above 0 (+INFINITY: no clipping).
 * sdc_get_actor / sdc_get_critic: the master copy in a host struct, with the flags (and the critic's scale and shift) as last set;
 * they wait for the device.  sdc_get_*_optim / sdc_set_*_optim: the moments and the state block to / from host memory (they wait for
 * the device); set refuses a step < 0, a power outside (0, 1], skipped < 0 and a moment that is not finite or a negative v.
 * sdc_set_critic_norm: the critic's scale and shift alone, ordered on `stream` (one small launch into SdcCriticDev) and into the
 * handle's host record; refused: scale not finite or <= 0, shift not finite (what sdc_set_critic refuses about them), no critic set. */
typedef struct {
  double lr, beta1, beta2, eps, weight_decay;
  double max_grad_norm;      /* > 0; +INFINITY means no clipping */
} sdc_adam;
typedef struct {
  int64_t step;              /* steps taken (skipped ones not counted) */
  double beta1_pow;          /* beta1 ** step and beta2 ** step as running fp64 products; both start at 1.0 */
  double beta2_pow;
  int64_t skipped;           /* steps refused on the device for a gradient that was not finite */
} sdc_optim_state;
int sdc_actor_adam_step(sdc_handle* h, int agent_slot, const float* grads, const sdc_adam* adam, double* grad_norm, void* stream);
int sdc_critic_adam_step(sdc_handle* h, const float* grads, const sdc_adam* adam, double* grad_norm, void* stream);
int sdc_get_actor(sdc_handle* h, int agent_slot, sdc_actor_params* out);
int sdc_get_critic(sdc_handle* h, sdc_critic_params* out);
int sdc_get_actor_optim(sdc_handle* h, int agent_slot, float* m, float* v, sdc_optim_state* st);
int sdc_set_actor_optim(sdc_handle* h, int agent_slot, const float* m, const float* v, const sdc_optim_state* st);
int sdc_get_critic_optim(sdc_handle* h, float* m, float* v, sdc_optim_state* st);
int sdc_set_critic_optim(sdc_handle* h, const float* m, const float* v, const sdc_optim_state* st);
int sdc_set_critic_norm(sdc_handle* h, double scale, double shift, void* stream);

/* TRAIN ON THE DEVICE.  replaces: what a trainer does between two collections around the calls above -- the shuffled mini-batches of
 * harl/common/buffers (feed_forward_generator_actor / _critic: torch.randperm(T N) per epoch, index sets of (T / num_mini_batch) N
 * rows) and harl/common/valuenorm.py ValueNorm.update, which v_critic.py cal_value_loss runs inside every critic mini-batch before it
 * normalises the returns with the new statistics.  Every call but the set / get pair is ordered on `stream` with no synchronisation
 * and no atomics: the same call gives the same bits on every run.  The arithmetic stands once, for the device and for a host
 * compiler, in csrc/sdc_minibatch.hpp; the kernels' plans: csrc/sdc_minibatch_dev.hpp.  The loop itself (agent order, epochs, the
 * HAPPO factor) is the binding's: dc_rl_amd.SdcEngine.happo_train.
 * sdc_permutation: perm[i], i < n, a keyed bijection of 0 .. n-1 (1 <= n <= 2^31 - 1) in int32 device memory, ONE launch of
 * sdc_permutation_kernel with one lane per output and no sort -- a six-round Feistel network over 4^b >= n values with cycle walking,
 * its round function one philox4x32_10 block (csrc/sdc_philox.hpp):
 *     bits = bit length of (n - 1)   (0 for n = 1);   b = max(1, (bits + 1) / 2);   mask = 2^b - 1
 *     x = i
 *     do {  L = x >> b;  R = x & mask
 *           for r = 0 .. 5:  F = philox4x32_10(counter (R, r, stream_lo, stream_hi), key (seed_lo, seed_hi)).x & mask;   (L, R) = (R, L ^ F)
 *           x = (L << b) | R
 *     } while (x >= n)
 *     perm[i] = x
 * (lo, hi: the low and high 32 bits of stream_id and seed).  For n >= 2, 4^b < 4 n: a lane walks fewer than four times on average.
 * IT IS A PSEUDO-RANDOM BIJECTION FOR SHUFFLING ROWS, NOT A UNIFORM DRAW FROM ALL n! PERMUTATIONS.  Four rounds are not enough: over
 * 4096 streams at n = 12 the position-by-value table has chi-square 234 on 121 degrees of freedom with four rounds and 129 with six.
 * Refused (-2 and a message, nothing enqueued): a null handle; n outside 1 .. 2^31 - 1; a null perm or one not dword-aligned.
 * sdc_gather_rows: for every k < n_rows and every segment g < n_segs (1 .. SDC_GATHER_MAX_SEGMENTS, a HOST array) the g.n_dwords
 * dwords at g.src + idx[k] * g.src_stride are copied to g.dst + k * g.dst_stride -- all arrays are dword arrays in device memory, the
 * strides are in dwords; ONE launch of sdc_gather_rows_kernel for all segments.  idx [n_rows] int32 device memory: a permutation,
 * a slice of one, or any index array.  The dwords between two destination rows keep their values.  AN INDEX OUTSIDE
 * [0, n_src_rows) IS NEVER AN ADDRESS: that destination row is written as zero dwords in every segment, and bad[0] (int32 device
 * memory, or NULL) receives a plain store of 1; bad is not cleared by the call.  Source and destination arrays must not overlap.
 * Refused: a null handle; n_rows < 1; n_src_rows outside 1 .. 2^31 - 1; a null idx or segs; idx or bad not dword-aligned; n_segs
 * outside 1 .. 16; a segment with a null src or dst, one not dword-aligned, n_dwords < 1 or a stride below n_dwords.
 * VALUENORM ON THE DEVICE: the handle keeps a device block {running_mean, running_mean_sq, debiasing_term, scale, shift} fp32 and a
 * host flag "installed".  sdc_set_value_norm installs the three values of `st` (NULL: uninstalls; the critic keeps the scale and shift
 * it has), derives, in fp32 with one rounding per operation,
 *     deb = max(debiasing_term, 1e-5);  mean = running_mean / deb;  mean_sq = running_mean_sq / deb
 *     var = max(mean_sq - mean * mean, 1e-2);  scale = sqrt(var);  shift = mean
 * and writes scale and shift into the critic's packed copy as sdc_set_critic_norm does; it waits for the device, as sdc_set_critic
 * does.  sdc_get_value_norm: the three values as the device holds them now (it waits for the device).  sdc_set_critic and
 * sdc_set_critic_norm do exactly what they did, and they UNINSTALL: a caller who sets scale and shift by hand has no running state.
 * While a ValueNorm is installed sdc_get_critic returns the device's scale and shift.
 * sdc_value_norm_update: ValueNorm.update for per_element_update = False over returns [n] fp32 device memory, TWO launches
 * (sdc_value_norm_sums_kernel, sdc_value_norm_update_kernel):
 *     S1 = sum of (double)x,  S2 = sum of (double)(float)(x * x)      // the square rounded to fp32 first, as the reference squares
 * both in sdc_ppo_terms' fixed two-stage order, word for word (B = min(ceil(n / 256), 1024) workgroups of 256 lanes, lane l of workgroup
 * b folds i = b * 256 + l + k * 256 * B from 0.0, the tree from 128 down; then one workgroup whose lane l takes partials l, l + 256,
 * ... and the same tree).  One lane then computes, each operation rounded once to fp32, nothing contracted:
 *     bm = (float)(S1 / n);  bsq = (float)(S2 / n);  w = (float)beta;  omw = (float)(1.0 - beta)      // the subtraction in double
 *     running_mean = running_mean * w + bm * omw;   running_mean_sq = running_mean_sq * w + bsq * omw
 *     debiasing_term = debiasing_term * w + omw
 * derives scale and shift as above, and stores the five values in the block and scale and shift in the critic's packed copy:
 * launches behind it on the stream -- sdc_critic_values, sdc_gae's value_preds, sdc_value_loss_normed -- see the new statistics.
 * Refused: a null handle; no critic set; no ValueNorm installed; n < 1; a null returns or one not dword-aligned; beta outside [0, 1).
 * sdc_value_loss_normed: sdc_value_loss with target_scale and target_shift read by the kernel from the block
 * (sdc_value_loss_normed_kernel: the same arithmetic, the same statistics, the same two launches); sdc_value_loss and its kernel are
 * unchanged.  Refused: what sdc_value_loss refuses about the arguments they share, and while no ValueNorm is installed. */
#define SDC_GATHER_MAX_SEGMENTS 16
typedef struct {
  float running_mean, running_mean_sq, debiasing_term;
} sdc_value_norm;
typedef struct {
  const void* src;           /* device memory, dword-aligned: row r starts at src + r * src_stride dwords */
  void* dst;                 /* device memory, dword-aligned: row k starts at dst + k * dst_stride dwords */
  long long src_stride, dst_stride;
  int n_dwords;              /* 1 .. min(src_stride, dst_stride) */
} sdc_gather_segment;
int sdc_permutation(sdc_handle* h, long long n, uint64_t seed, uint64_t stream_id, int32_t* perm, void* stream);
int sdc_gather_rows(sdc_handle* h, const int32_t* idx, long long n_rows, long long n_src_rows, const sdc_gather_segment* segs, int n_segs,
                    int32_t* bad, void* stream);
int sdc_set_value_norm(sdc_handle* h, const sdc_value_norm* st);
int sdc_get_value_norm(sdc_handle* h, sdc_value_norm* out);
int sdc_value_norm_update(sdc_handle* h, const float* returns, long long n, double beta, void* stream);
int sdc_value_loss_normed(sdc_handle* h, long long n, const float* raw_values, const float* value_preds, const float* returns,
                          double clip_param, double huber_delta, int flags, double coef, float* loss, float* dvalue, double* stats,
                          void* stream);

/* PLAN FORECAST: what the plan calls' rollouts believe the traces of the next n_steps steps are.  Without one a plan call's rollouts
 * read the episode's own feature rows -- the real workload, carbon intensity, dry bulb (with the weather noise the episode drew) and wet
 * bulb of the steps ahead: perfect foresight, an oracle bound.  A forecast is host state of the handle: sdc_set_plan_forecast copies the
 * struct (not the array `values` points to), and every later sdc_plan, sdc_plan_cem and sdc_plan_cem_groups call plans against it until it
 * is cleared (fc NULL); neither call touches the device.  sdc_get_plan_forecast copies out what is set (cleared: every field 0).
 * With i an env's trace-table index and rel its episode step when the plan call starts, K = n_steps and J = K + 2, the forecast is
 * fc[j][n][c], fp64, j = 0 .. J - 1, c in (W, C, T, WB) = (workload, carbon intensity, dry bulb, wet bulb): what the planner believes
 * trace c is at table index i + j.  Each channel has a mode:
 *   SDC_FORECAST_PERFECT      the truth: W, C = table[loc][clamp(i + j, 0, SDC_TABLE_LEN - 1)]; T, WB = t_win / wb_win[n][rel + j].  The
 *                             channel's slots are NOT WRITTEN.
 *   SDC_FORECAST_PERSISTENCE  the truth at j = 0, for every j
 *   SDC_FORECAST_DAILY        j = 0: the truth; j >= 1: the truth 96 indices earlier (table[clamp(i + j - 96)]; win[rel + j - 96]) --
 *                             where rel + j < 96, T and WB fall back to persistence (the windows start at the episode's first index)
 *   SDC_FORECAST_VALUES       values[j][n][c] (device, fp64, [values_entries][N][4]), as given: not clipped (a workload outside [0, 1]
 *                             raises SDC_FAULT_WORKLOAD in the rollouts, as a step does).  Read at every plan call: the caller
 *                             refreshes the contents between decisions
 * Between its mark and its return a plan call OVERLAYS the step inputs in the feature rows rel + 1 .. rel + K of every env (row
 * rel + 1 + k holds the inputs of the step from episode step rel + k): W, C, T, WB = fc[k]; T1 = (float) fc[k + 1].T;
 * NCNEXT = (fc[k + 2].C - ci_min) / ci_den from the env's record (an IEEE subtraction, then an IEEE division) -- only the slots of
 * channels that are not PERFECT -- and puts the saved bits back before it returns, whatever its return code: three more launches per call
 * (sdc_forecast_fill_kernel, sdc_forecast_swap_kernel twice; csrc/sdc_forecast.hip), none with every channel PERFECT or no forecast
 * set.  The rows' observation entries stay the truth: a slot on a built-in rule-based policy keeps reading the true observation
 * features.  Replicas of a group (sdc_plan_cem_groups) get identical rows from the built-in modes by construction; VALUES must be
 * identical within a group, which is the caller's duty.
 * sdc_forecast_traces: one launch of the fill kernel alone -> out[j][n][c], j < n_entries: what the handle's forecast gives from the
 * current state, or the true traces when truth != 0 (how a caller builds VALUES: truth plus its own error model).
 * Refused (-2 and a message; the forecast set before stays in force): sdc_set_plan_forecast: a null handle, a mode outside 0..3, a
 * negative values_entries.  sdc_forecast_traces: a null handle or out, n_entries outside [1, SDC_MARK_MAX_STEPS + 2] or above
 * sdc_steps_to_episode_end() + 2, no reset yet, a VALUES channel (truth == 0) with null values or values_entries < n_entries.  The plan
 * calls, while a channel is not PERFECT: an engine without feature rows or an env whose rows are not valid (after a host write to its
 * state), a VALUES channel with null values or values_entries < n_steps + 2. */
#define SDC_FORECAST_PERFECT 0
#define SDC_FORECAST_PERSISTENCE 1
#define SDC_FORECAST_DAILY 2
#define SDC_FORECAST_VALUES 3
typedef struct {
  int32_t mode[4];          /* SDC_FORECAST_* of W, C, T, WB */
  int32_t values_entries;   /* entries j of `values` (VALUES channels: >= n_steps + 2 at a plan call) */
  const double* values;     /* [values_entries][N][4] device, or NULL */
} sdc_plan_forecast;
int sdc_set_plan_forecast(sdc_handle* h, const sdc_plan_forecast* fc);
int sdc_get_plan_forecast(const sdc_handle* h, sdc_plan_forecast* out);
int sdc_forecast_traces(sdc_handle* h, int n_entries, int truth, double* out, void* stream);

/* PLAN WITH THE CROSS-ENTROPY METHOD: n_iters rounds of "sample n_cand candidate sequences from a per-env, per-step, per-agent
 * categorical distribution, score them as sdc_plan does, refit the distribution to the n_elite best and keep the best sequence found so
 * far" -- one call, ordered on `stream`, no device synchronisation, ONE mark of the whole batch (max_steps = n_steps) for all n_iters *
 * n_cand rollouts.  Per iteration it = iter0 .. iter0 + n_iters - 1: sdc_cem_sample_kernel; sdc_plan's own per-candidate loop (rollout
 * into the handle's output block, sdc_plan_score_kernel, rewind; the objective, its arithmetic and the chunking are sdc_plan's);
 * sdc_cem_refit_kernel.  Afterwards the engine is where sdc_plan leaves it (rewound, re-centring stamps cleared, the caller's output
 * arrays never written), and THE CALL USES UP THE ENVS' ONE LIVE MARK.  All arrays are the device's; K = n_steps, M = n_cand,
 * E = n_elite, I = n_iters, N the batch:
 *   probs       in/out [K][N][3 agents][3 actions] fp64     best_seq    in/out [K][N][3] int32: the incumbent on entry, the best
 *   best_score  out [I][N]: the incumbent's score after each iteration        sequence found on return
 *   best_action out [N][3] = best_seq[0]                    cand        work/out [M][K][N][3]: the last iteration's candidates
 *   cand_score  work/out [M][N]: their scores
 * SAMPLE.  Candidate 0 is a copy of best_seq (elitism: the incumbent's score never falls from one iteration to the next, and it wins
 * ties).  For m = 1 .. M-1, step k, env n: one philox4x32_10 block with counter (m * K + k, env_index_base + n, draw, (it << 16) |
 * 0xCE3D) and key (seed's low word, seed's high word); words x, y, z serve agents ls, dc, bat, w is unused.  For agent a with
 * probabilities p0, p1, p2:  u = (double)word * 2^-32;  action = (u >= p0) + (u >= (p0 + p1)) -- one fp64 addition; p2 is never read.
 * fixed_action[a] >= 0 replaces the draw of agent a in candidates 1 .. M-1.
 * REFIT, per env.  rank(c) = the number of c' with score[c'] > score[c], or score[c'] == score[c] and c' < c; c is elite iff rank(c) <
 * E; best = the candidate of rank 0.  best_seq[:][n] = candidate best's actions (best = 0: unchanged), best_score[it - iter0][n] =
 * score[best][n], and after the last iteration best_action[n] = best_seq[0][n].  For every step k and agent a without a fixed action,
 * with cnt[j] the number of elites whose action is j, all fp64, no fused multiply-adds, an IEEE division:
 *   t_j = (double)cnt[j] / (double)E;  q_j = alpha * p_j + take * t_j  (take = 1.0 - alpha, computed once on the host);
 *   q_j = max(q_j, p_min);  s = (q0 + q1) + q2;  p_j = q_j / s
 * An agent with a fixed action keeps its probs.
 * THE ENTRIES OF probs AND best_seq ARE NOT VALIDATED: they live on the device.  Probabilities that are not a distribution give
 * whatever the thresholds above give; an action outside 0..2 is played as sdc_rollout plays it.  A NaN score (a non-finite objective) is
 * outranked by nothing and outranks nothing: every such candidate has rank 0 and is elite, so the elites may then be more than E while
 * the divisor stays E; best is the lowest-numbered candidate of rank 0, so the result is still the same from run to run.
 * Refused (-2 and a message, nothing enqueued, the engine untouched): everything sdc_plan refuses, with the same horizon, auto-reset and
 * verify-mode rules; a null cem; n_iters < 1, iter0 < 0, iter0 + n_iters > 65536; n_cand outside [2, SDC_CEM_MAX_CAND]; n_elite outside
 * [1, n_cand]; a fixed_action outside [-1, 2]; alpha outside [0, 1); p_min outside [0, 1/3]; a null array. */
#define SDC_CEM_MAX_CAND 64
typedef struct {
  int32_t n_iters;          /* I >= 1 */
  int32_t iter0;            /* index of this call's first iteration, >= 0, iter0 + I <= 65536 */
  int32_t n_cand;           /* M in [2, SDC_CEM_MAX_CAND] */
  int32_t n_elite;          /* E in [1, M] */
  int32_t fixed_action[3];  /* per agent: -1 = sampled, 0..2 = every sampled candidate carries this value */
  uint32_t draw;            /* the caller's decision counter: goes into the generator's counter */
  uint64_t seed;
  double alpha;             /* [0, 1): weight of the old distribution in the refit */
  double p_min;             /* [0, 1/3]: floor of every probability before renormalising */
} sdc_cem_params;
int sdc_plan_cem(sdc_handle* h, int n_steps, const sdc_cem_params* cem, const sdc_plan_objective* objective, double* probs,
                 int32_t* best_seq, double* best_score, int32_t* best_action, int32_t* cand, double* cand_score, float* obs,
                 float* share_obs, void* stream);

/* PLAN WITH THE CROSS-ENTROPY METHOD OVER REPLICA GROUPS: sdc_plan_cem with the candidates in env slots instead of one after another in
 * time.  The batch of N = G * R envs is G groups of R = group_size consecutive envs (replicas): group g = envs [g R, (g + 1) R).  THE R
 * REPLICAS OF A GROUP HOLD THE SAME STATE -- the caller's contract (sdc_clone_envs from the group's first env makes it so, and stepping
 * every replica with step_actions keeps it so).  What the host mirrors know is checked (below); bit equality of the replicas' states
 * beyond that is NOT validated on the device: replicas that differ are scored from their own states.  In one iteration every replica
 * plays its own sampled sequence in ONE rollout of the whole batch, and the distribution is refitted per group: per iteration it =
 * iter0 .. iter0 + n_iters - 1 one sdc_cem_group_sample_kernel, sdc_plan's per-candidate path with the single "candidate" cand (rollout
 * into the handle's output block in chunks, sdc_plan_score_kernel, rewind; the objective, its arithmetic, the chunking and debug_flags
 * bit 14 are sdc_plan's), one sdc_cem_group_refit_kernel -- whatever R is.  One call, ordered on `stream`, no device synchronisation,
 * ONE mark of the whole batch (max_steps = n_steps).  Afterwards the engine is where sdc_plan_cem leaves it (rewound, re-centring stamps
 * cleared, the caller's output arrays never written), and THE CALL USES UP THE ENVS' ONE LIVE MARK.  All arrays are the device's; K =
 * n_steps, E = n_elite, I = n_iters:
 *   probs        in/out [K][G][3 agents][3 actions] fp64    best_seq     in/out [K][G][3] int32: the incumbent on entry, the best
 *   best_score   out [I][G]: the incumbent's score after each iteration        sequence found on return
 *   best_action  out [G][3] = best_seq[0]                   step_actions out [N][3] = best_action[n / R]: what to hand to sdc_step so
 *   cand         work/out [K][N][3], sdc_rollout's `actions` layout: replica r of group g plays         that a group stays identical
 *   cand[:][g R + r]; the last iteration's                  cand_score   work/out [N]: their scores
 * The arithmetic is sdc_plan_cem's with "candidate m of env n" read as "replica r of group g":
 * SAMPLE.  Replica 0 carries a copy of best_seq (the incumbent: its score never falls from one iteration to the next, and it wins
 * ties).  For r = 1 .. R-1, step k, group g: one philox4x32_10 block with counter (r * K + k, group_base + g, draw, (it << 16) |
 * 0xCE3D) and key (seed's low word, seed's high word); words x, y, z serve agents ls, dc, bat, w is unused.  For agent a with
 * probabilities p0, p1, p2:  u = (double)word * 2^-32;  action = (u >= p0) + (u >= (p0 + p1)) -- one fp64 addition; p2 is never read.
 * fixed_action[a] >= 0 replaces the draw of agent a in replicas 1 .. R-1.
 * REFIT, per group over its R scores s[r] = cand_score[g R + r].  rank(r) = the number of r' with s[r'] > s[r], or s[r'] == s[r] and
 * r' < r; r is elite iff rank(r) < E; best = the lowest-numbered replica of rank 0.  best_seq[:][g] = replica best's actions (best = 0:
 * the bits it had), best_score[it - iter0][g] = s[best], and after the last iteration best_action[g] = best_seq[0][g] and
 * step_actions[g R + r] = best_action[g] for every r.  For every step k and agent a without a fixed action, with cnt[j] the number of
 * elites whose action (its low two bits) is j, all fp64, no fused multiply-adds, an IEEE division:
 *   t_j = (double)cnt[j] / (double)E;  q_j = alpha * p_j + take * t_j  (take = 1.0 - alpha, computed once on the host);
 *   q_j = max(q_j, p_min);  s = (q0 + q1) + q2;  p_j = q_j / s
 * An agent with a fixed action keeps its probs.  The entries of probs and best_seq are not validated, and a NaN score is outranked by
 * nothing and outranks nothing (rank 0, elite; the divisor stays E), both as in sdc_plan_cem.
 * CONSEQUENCE: an engine of G envs running sdc_plan_cem with n_cand = R <= SDC_CEM_MAX_CAND and env_index_base = group_base, and an
 * engine of G R envs whose group g holds that engine's env g, return the same probs, best_seq, best_score and best_action bit for
 * bit, and the latter's cand_score[g R + r] is the former's cand_score[r][g].
 * Refused (-2 and a message, nothing enqueued, the engine untouched): everything sdc_plan_cem refuses, with n_cand read as group_size
 * (a null params; n_iters < 1, iter0 < 0, iter0 + n_iters > 65536; a fixed_action outside [-1, 2]; alpha outside [0, 1); p_min outside
 * [0, 1/3]; sdc_plan's horizon, auto-reset and verify-mode rules; a null array); group_size outside [2, SDC_CEM_MAX_GROUP]; n_envs not
 * a multiple of group_size; n_elite outside [1, group_size]; group_base < 0; and, from the host mirrors in O(N), a group whose replicas
 * are not all at the same episode step, data-centre config, location and feature-row flag. */
#define SDC_CEM_MAX_GROUP 1024
typedef struct {
  int32_t group_size;       /* R in [2, SDC_CEM_MAX_GROUP]; N % R == 0; group g = envs [g R, (g+1) R) */
  int32_t group_base;       /* global index of this engine's group 0, >= 0: goes into the generator's counter */
  int32_t n_iters;          /* I >= 1 */
  int32_t iter0;            /* index of this call's first iteration, >= 0, iter0 + I <= 65536 */
  int32_t n_elite;          /* E in [1, R] */
  int32_t fixed_action[3];  /* per agent: -1 = sampled, 0..2 = every sampled replica carries this value */
  uint32_t draw;            /* the caller's decision counter: goes into the generator's counter */
  uint64_t seed;
  double alpha;             /* [0, 1): weight of the old distribution in the refit */
  double p_min;             /* [0, 1/3]: floor of every probability before renormalising */
} sdc_cem_group_params;
int sdc_plan_cem_groups(sdc_handle* h, int n_steps, const sdc_cem_group_params* cem, const sdc_plan_objective* objective, double* probs,
                        int32_t* best_seq, double* best_score, int32_t* best_action, int32_t* step_actions, int32_t* cand,
                        double* cand_score, float* obs, float* share_obs, void* stream);

/* EPISODE STATISTICS: advance the engine by n_steps env-steps exactly as sdc_rollout(h, n_steps, actions, ...) would -- the call is made
 * of sdc_rollout calls: the same kernel choice, launch counter and host mirrors, the auto-reset at the episode's end -- and hand back
 * per-env statistics of the steps' outputs instead of the outputs.  No mark, no rewind: the engine moves.  One call, ordered on `stream`,
 * no device synchronisation (the handle's output block is allocated on first use and when it has to grow).  The rollouts write into the
 * output block the handle owns (sdc_plan's: capped at 256 MiB, csrc/sdc_plan.hpp) in chunks of as many steps as fit, at least one;
 * debug_flags bit 14 (TEST HOOK): two steps.  After each chunk one launch of sdc_stats_reduce_kernel (csrc/sdc_stats.hip) folds the
 * chunk's info and rew rows into stats / returns / counts; after the last chunk sdc_stats_last_kernel copies the last step's obs,
 * share_obs, rew, done and info rows to the caller's single-step arrays [N]... (obs and share_obs required; rew, done, info, final_obs
 * may be NULL), and the block's final_obs rows of the envs that finished into final_obs (the other rows keep what they held, as after
 * sdc_rollout).  n_steps may reach the episode's end -- the statistics cover the n_steps steps taken, the terminal one included, and
 * obs / share_obs then hold the reset observations as after sdc_rollout -- and is not limited by SDC_MARK_MAX_STEPS.
 * actions [n_steps][N][3] int32 (device); NULL when every slot has a built-in policy.  All arrays are the device's:
 *   stats   [SDC_STATS_FIELDS][N][SDC_INFO_DIM] fp64, 16-byte aligned      returns [N][3] fp64, 16-byte aligned
 *   counts  [N][2] int32: steps reduced, the OR of the steps' info[fault] bits
 * accumulate == 0:  SUM = 0.0, MIN = +inf, MAX = -inf, NPOS = 0.0, returns = 0.0, counts = 0;  accumulate == 1: continue from what the
 * arrays hold.  Then for k = 0 .. n_steps - 1 in order, all in fp64 without fused multiply-adds, per env n and info column c with
 * x = (double)info_k[n][c]:
 *   SUM += x;   MIN = x < MIN ? x : MIN;   MAX = x > MAX ? x : MAX;   NPOS += (x > 0.0) ? 1.0 : 0.0
 *   returns[n][a] += (double)rew_k[n][a];   counts[n][0] += 1;   counts[n][1] |= (uint32_t)info_k[n][SDC_INFO_FAULT]
 * A NaN therefore never enters MIN, MAX or NPOS and propagates through SUM.  All 44 columns are reduced.  The results depend neither on
 * the chunking nor on splitting one call into several with accumulate == 1.
 * Refused (-2 and a message, nothing enqueued, the engine untouched): a null handle; n_steps < 1; a null stats / returns / counts / obs /
 * share_obs; stats or returns not 16-byte aligned, another array not dword-aligned; accumulate outside {0, 1}; no sdc_reset yet; verify
 * mode (debug_flags bit 0), which sdc_rollout refuses as well; null actions while a slot is on SDC_POLICY_EXTERNAL; n_steps >
 * sdc_steps_to_episode_end(). */
#define SDC_STATS_FIELDS 4
enum sdc_stat_field { SDC_STAT_SUM = 0, SDC_STAT_MIN, SDC_STAT_MAX, SDC_STAT_NPOS };
int sdc_rollout_stats(sdc_handle* h, int n_steps, const int32_t* actions, int accumulate, double* stats, double* returns,
                      int32_t* counts, float* obs, float* share_obs, float* rew, uint8_t* done, float* info, float* final_obs,
                      void* stream);

/* POLICY EVALUATION: advance the engine by n_steps env-steps exactly as sdc_rollout_actor(h, n_steps, sample, ...) would -- the call is
 * made of sdc_rollout_actor calls: the same kernel choice, launch counter, host mirror and observation latch, the same draws for
 * sample = 1, the auto-reset at the episode's end -- and hand back statistics instead of outputs: sdc_rollout_stats' per-env statistics
 * of the environment's outputs, and per env and agent what the actors did.  No mark, no rewind: the engine moves.  One call, ordered on
 * `stream`, no device synchronisation (the handle's buffers are allocated on first use and when they have to grow).  The rollouts write
 * into the output block the handle owns (sdc_plan's, as for sdc_rollout_stats) in chunks of as many steps as fit, at least one;
 * debug_flags bit 14 (TEST HOOK): two steps; the chunk's actions and logits go into a second buffer of the handle's, chunk x N x 48
 * bytes.  After each chunk one launch of sdc_stats_reduce_kernel folds the chunk's info and rew rows into stats / returns / counts and,
 * when the policy arrays are given, one launch of sdc_policy_stats_kernel (csrc/sdc_policy_stats.hip) folds its actions and logits into
 * them; after the last chunk sdc_stats_last_kernel fills the caller's single-step arrays as for sdc_rollout_stats.
 * stats, returns, counts, accumulate and the single-step arrays: sdc_rollout_stats' contract and arithmetic, word for word.
 * The policy arrays are the device's, and either both or neither is given:
 *   policy_counts [N][3][SDC_POLICY_COUNTS] int32: per env and agent N0, N1, N2 (steps on which action 0 / 1 / 2 was played), SWITCHES
 *                 (steps whose action differs from the step before), LAST (the last action; -1: none yet)
 *   policy_sums   [N][3][SDC_POLICY_SUMS] fp64, 16-byte aligned: LOGP (the summed log-probability of the actions played), ENTROPY (the
 *                 summed entropy of the distributions they were chosen from)
 * accumulate == 0:  N0 = N1 = N2 = SWITCHES = 0, LAST = -1, LOGP = ENTROPY = 0.0;  accumulate == 1: continue from what the arrays hold.
 * Then for k = 0 .. n_steps - 1 in order, per env n and agent a, with j the action and l0, l1, l2 the fp32 logits of that step:
 *   N_j += 1;   SWITCHES += (LAST >= 0 && j != LAST) ? 1 : 0;   LAST = j
 *   m = max(l0, l1, l2) in fp32;   z_i = (double)l_i - (double)m;   e_i = exp(z_i);   s = (e0 + e1) + e2;   lse = log(s)
 *   lp_i = z_i - lse;   p_i = e_i / s
 *   LOGP += lp_j;   ENTROPY += -((p0 * lp0 + p1 * lp1) + p2 * lp2)
 * all in fp64 without fused multiply-adds.  Nothing special happens at an episode boundary: a caller who wants per-episode numbers
 * starts each episode with accumulate == 0.  The results depend neither on the chunking nor on splitting one call into several with
 * accumulate == 1.
 * Refused (-2 and a message, nothing enqueued, the engine untouched), all before the first chunk's launch: what sdc_rollout_stats refuses
 * except what concerns `actions` (a null handle; n_steps < 1; a null stats / returns / counts / obs / share_obs; stats or returns not
 * 16-byte aligned, another array not dword-aligned; accumulate outside {0, 1}; no sdc_reset yet; verify mode; n_steps >
 * sdc_steps_to_episode_end()); what sdc_rollout_actor refuses (an actor not set; the three activations not equal; no observations yet;
 * a batch that is not the common case); sample outside {0, 1}; one policy array without the other; policy_sums not 16-byte aligned;
 * policy_counts not dword-aligned. */
#define SDC_POLICY_COUNTS 5
enum sdc_policy_count { SDC_POLICY_N0 = 0, SDC_POLICY_N1, SDC_POLICY_N2, SDC_POLICY_SWITCHES, SDC_POLICY_LAST };
#define SDC_POLICY_SUMS 2
enum sdc_policy_sum { SDC_POLICY_LOGP = 0, SDC_POLICY_ENTROPY };
int sdc_rollout_actor_stats(sdc_handle* h, int n_steps, int sample, int accumulate, double* stats, double* returns, int32_t* counts,
                            int32_t* policy_counts, double* policy_sums, float* obs, float* share_obs, float* rew, uint8_t* done,
                            float* info, float* final_obs, void* stream);

/* PLANNER EVALUATION: advance the engine by n_steps env-steps under receding-horizon control with the cross-entropy method -- before
 * every step the library plans exactly as sdc_plan_cem does and then plays the first action of the best sequence found -- and hand back
 * sdc_rollout_stats' per-env statistics of the steps taken, per env and agent what the planner played, and per env what it predicted.
 * One call, ordered on `stream`, no device synchronisation (the handle's buffers are allocated on first use and when they have to grow)
 * and no host wait between the decisions: the discount table of the whole call is staged once.  The engine ends where n_steps rounds of sdc_plan_cem followed
 * by a one-step sdc_rollout_stats of best_action would leave it, the auto-reset at the episode's end included, and THE CALL USES UP THE
 * ENVS' ONE LIVE MARK, as every plan call does.  The handle's plan terms and plan forecast apply to every decision.
 * THE DECISION SCHEDULE (csrc/sdc_mpc_schedule.hpp).  H = mpc->horizon; for step t of the call let `left` be
 * sdc_steps_to_episode_end() before that step and K_t = min(H, auto_reset ? left - 1 : left).  The decision is PLANNED iff left >= 2 and
 * K_t >= 1; otherwise it is IDLE: idle_action is played, no draw is consumed and the carried distribution is dropped.  A planned
 * decision starts FRESH -- probs = 1.0 / 3.0 (the double) everywhere, best_seq = idle_action -- when warm_start == 0; when it is the
 * call's first planned decision and resume == 0; when the decision before it was idle; and when K_t exceeds the number of steps the
 * carried result has.  Otherwise it starts from the carried result SHIFTED: steps 0 .. K_t - 2 take steps 1 .. K_t - 1, step K_t - 1 is
 * uniform / idle_action.  resume == 1: probs / best_seq hold an earlier decision's unshifted result of resume_steps steps.  The j-th
 * planned decision of the call (j = 0, 1, ...) is sdc_plan_cem with n_steps = K_t, the embedded cem parameters and draw = cem.draw + j
 * (mod 2^32).  After the call probs[0:K] and best_seq[0:K] hold the last planned decision's result, unshifted, K its horizon; after a
 * call whose last decision was idle they hold nothing a later call may resume from.
 * PER STEP, in stream order: a planned decision is one sdc_mpc_start_kernel (csrc/sdc_mpc.hip: the fresh fill or the in-place shift),
 * sdc_plan_cem's own launches (mark, I x (sample, M x (rollout, score, rewind), refit), the forecast's overlay) and one
 * sdc_mpc_fold_kernel; an idle decision is one sdc_mpc_fold_kernel, which writes idle_action into best_action.  Then the step:
 * sdc_rollout of one step with best_action into the handle's output block, and sdc_stats_reduce_kernel behind it; behind the call's
 * last step sdc_stats_last_kernel fills the single-step arrays as for sdc_rollout_stats.  The planner's rollouts share the block with the
 * step: the stream orders them.
 * stats, returns, counts, accumulate and the single-step arrays: sdc_rollout_stats' contract and arithmetic, word for word.  The
 * planner's arrays are sdc_plan_cem's with K read as H -- probs [H][N][3][3], best_seq [H][N][3], best_score [I][N], best_action [N][3],
 * cand [M][H][N][3], cand_score [M][N] --; a decision with K < H uses the contiguous [K]... prefix of each, so best_score, cand and
 * cand_score hold the last planned decision's and best_action the last action played.  The plan statistics are the device's, and
 * either both or neither is given:
 *   plan_counts [N][3][SDC_POLICY_COUNTS] int32, sdc_policy_count's entries of the actions PLAYED, idle decisions included: with j the
 *               action,  N_j += 1;  SWITCHES += (LAST >= 0 && j != LAST) ? 1 : 0;  LAST = j
 *   plan_sums   [N][SDC_PLAN_SUMS] fp64, 16-byte aligned: on a planned decision  SCORE += best_score[I-1][n];  GAIN +=
 *               best_score[I-1][n] - best_score[0][n];  PLANNED += 1.0;  on an idle one  IDLE += 1.0  and nothing else.  fp64, in
 *               step order, no fused operation
 * accumulate == 0:  N0 = N1 = N2 = SWITCHES = 0, LAST = -1, the sums 0.0;  accumulate == 1: continue from what the arrays hold.
 * Refused (-2 and a message, nothing enqueued, the engine untouched), all before the first launch: what sdc_rollout_stats refuses except
 * what concerns `actions` (n_steps > sdc_steps_to_episode_end() among it); what sdc_plan_cem refuses about its parameters, objective and
 * arrays (its horizon and auto-reset rules are replaced by the schedule above; a forecast's needs are asked for the longest decision);
 * a null mpc; horizon outside [1, SDC_MARK_MAX_STEPS]; warm_start or resume outside {0, 1}; resume_steps outside [1, horizon] while
 * resuming; an idle_action outside 0..2; one of plan_counts / plan_sums without the other; plan_sums not 16-byte aligned; probs or
 * best_score or cand_score not 8-byte aligned, plan_counts or another int32 array not dword-aligned. */
#define SDC_PLAN_SUMS 4
enum sdc_plan_sum { SDC_PLAN_SCORE = 0, SDC_PLAN_GAIN, SDC_PLAN_PLANNED, SDC_PLAN_IDLE };
typedef struct {
  int32_t horizon;         /* H in [1, SDC_MARK_MAX_STEPS] */
  int32_t warm_start;      /* 0: every planned decision starts fresh; 1: from the carried result shifted where the schedule allows */
  int32_t resume;          /* 1: probs / best_seq hold an earlier decision's unshifted result */
  int32_t resume_steps;    /* ... of this many steps, in [1, H] (read only while resuming) */
  int32_t idle_action[3];  /* each 0..2: what an idle decision plays, and a fresh best_seq */
  int32_t reserved;
  sdc_cem_params cem;      /* sdc_plan_cem's parameters; draw: the first planned decision's */
} sdc_mpc_params;
int sdc_rollout_cem_stats(sdc_handle* h, int n_steps, const sdc_mpc_params* mpc, const sdc_plan_objective* objective, int accumulate,
                          double* stats, double* returns, int32_t* counts, int32_t* plan_counts, double* plan_sums, double* probs,
                          int32_t* best_seq, double* best_score, int32_t* best_action, int32_t* cand, double* cand_score, float* obs,
                          float* share_obs, float* rew, uint8_t* done, float* info, float* final_obs, void* stream);

/* PLANNER EVALUATION OVER REPLICA GROUPS: sdc_rollout_cem_stats with every planned decision replaced by sdc_plan_cem_groups' own body --
 * the batch is G = N / R groups of R = cem.group_size consecutive envs that hold one state, one iteration is ONE rollout of the batch --
 * and, behind every step, a check on the device that a group's replicas still agree.  One call, ordered on `stream`, no device
 * synchronisation and no host wait between the decisions; the discount table of the whole call is staged once; the handle's plan terms
 * and plan forecast apply to every decision; THE CALL USES UP THE ENVS' ONE LIVE MARK.  The engine ends where -- after the sync below --
 * n_steps rounds of sdc_plan_cem_groups followed by a one-step sdc_rollout_stats of step_actions would leave it.
 * sync_first == 1: the call begins with one sdc_clone_envs of the batch, the groups' first envs g R as sources and the envs g R + 1 ..
 * g R + R - 1 as destinations (the caller's obs / share_obs rows follow), and the first planned decision starts fresh; the O(N) check
 * of the host mirrors that sdc_plan_cem_groups makes ("group out of step") is skipped, the clone establishes it, and the episode's end
 * is the groups' first envs'.  sync_first == 0: the check is made as sdc_plan_cem_groups makes it.  n_steps <=
 * sdc_steps_to_episode_end() lets an auto-reset happen at the call's last step only -- the replicas draw resets of their own there --,
 * so one sync at the front of a call is all a whole episode needs; the next call syncs again.
 * THE DECISION SCHEDULE is sdc_rollout_cem_stats' (csrc/sdc_mpc_schedule.hpp), unchanged; the j-th planned decision of the call is
 * sdc_plan_cem_groups with n_steps = K_t, the embedded cem parameters and draw = cem.draw + j (mod 2^32).
 * PER STEP, in stream order: a planned decision is one sdc_mpc_start_kernel over the G groups, sdc_plan_cem_groups' own launches (mark,
 * I x (group sample, rollout, score, rewind, group refit), the forecast's overlay) and -- with the plan statistics -- one
 * sdc_mpc_group_fold_kernel (csrc/sdc_mpc_groups.hip); an idle decision is one sdc_mpc_group_fold_kernel, which writes idle_action into
 * best_action and into every row of step_actions.  Then the step: sdc_rollout of one step with step_actions into the handle's output
 * block, sdc_stats_reduce_kernel behind it and -- with the plan statistics -- sdc_group_agree_kernel over the same rows; behind the
 * call's last step sdc_stats_last_kernel fills the single-step arrays as for sdc_rollout_stats.
 * stats, returns, counts [N]..., accumulate and the single-step arrays: sdc_rollout_stats' contract and arithmetic, word for word, per
 * env: a group's replicas carry equal rows, and the caller reads every R-th.  The planner's arrays are sdc_plan_cem_groups' with K read
 * as H -- probs [H][G][3][3], best_seq [H][G][3], best_score [I][G], best_action [G][3], step_actions [N][3], cand [H][N][3], cand_score
 * [N] --; a decision with K < H uses the contiguous [K]... prefix of each.  The plan statistics are the device's, and all three or none
 * are given:
 *   plan_counts [G][3][SDC_POLICY_COUNTS], plan_sums [G][SDC_PLAN_SUMS] (16-byte aligned): sdc_rollout_cem_stats' entries and
 *               arithmetic with "env n" read as "group g" (the action played is best_action[g], the scores best_score[.][g])
 *   diverged    [G] int32: the number of (step, replica) pairs of the call at which replica n = g R + r, r >= 1, differed from its
 *               group's first env in ANY BIT of the step's three rew dwords, its done byte or its info row without info[reserved]
 *               (scheduling-dependent by definition).  obs is not compared: after the terminal step it holds the replicas' own reset
 *               observations.  accumulate == 0: from 0; accumulate == 1: from what it holds.
 * Refused (-2 and a message, nothing enqueued, the engine untouched), all before the first launch: what sdc_rollout_cem_stats refuses
 * (with sdc_plan_cem's n_cand rules replaced by the following); what sdc_plan_cem_groups refuses about group_size, n_elite and
 * group_base, and -- sync_first == 0 -- a group out of step; sync_first outside {0, 1}; sync_first together with resume; one of
 * plan_counts / plan_sums / diverged without the others; step_actions null or, like diverged, not dword-aligned. */
typedef struct {
  int32_t horizon;           /* as sdc_mpc_params */
  int32_t warm_start;
  int32_t resume;
  int32_t resume_steps;
  int32_t idle_action[3];
  int32_t sync_first;        /* 1: before the first decision every group becomes a copy of its first env */
  sdc_cem_group_params cem;  /* sdc_plan_cem_groups' own; draw: the first planned decision's */
} sdc_mpc_group_params;
int sdc_rollout_cem_groups_stats(sdc_handle* h, int n_steps, const sdc_mpc_group_params* mpc, const sdc_plan_objective* objective,
                                 int accumulate, double* stats, double* returns, int32_t* counts, int32_t* plan_counts, double* plan_sums,
                                 int32_t* diverged, double* probs, int32_t* best_seq, double* best_score, int32_t* best_action,
                                 int32_t* step_actions, int32_t* cand, double* cand_score, float* obs, float* share_obs, float* rew,
                                 uint8_t* done, float* info, float* final_obs, void* stream);

/* Per-kernel timing (measurement only; off by default).  enable = k > 0 samples every k-th sdc_step, 0 switches it
 * off.  In a sampled step one lane per workgroup of each kernel stamps the device's constant-rate wall clock at
 * entry and exit; sdc_profile_read synchronises the device and accumulates, per sampled launch,
 * max(exit) - min(entry) over the workgroups -- the launch's duration on the GPU, with no host-event overhead.
 *   out[0] = sdc_dynamics_kernel (the step kernel) total ms, out[1] = 0 (no separate reward kernel any more),
 *   out[2] = sdc_reset_kernel (auto-reset) total ms, out[3] = steps sampled, out[4] = auto-resets sampled. */
int sdc_profile_enable(sdc_handle* h, int enable);
int sdc_profile_read(sdc_handle* h, double* out5, int reset);

#ifdef __cplusplus
}
#endif
#endif
