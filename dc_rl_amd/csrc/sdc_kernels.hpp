// sdc_kernels.hpp -- every kernel that is defined in one file and launched from another (sdc_capi.hip), declared ONCE.
//
// The kernels are extern "C": the linker compares names, not argument lists, so a prototype retyped at the launch site would link and
// launch with a shifted argument block once the definition changes.  The launch site AND each defining file include this header; a
// definition that differs from its declaration here is then a compile error ("conflicting types").  The definition adds its own
// attributes (__launch_bounds__, amdgpu_waves_per_eu, __restrict__, top-level const) behind the plain declaration.
// The newer kernels (clone, snapshot, mark, plan, cem, stats) are launched from their own files: their *_launch functions are declared
// next to their plans (sdc_clone.hpp, ...).
#pragma once

#include "sdc_device.hpp"

struct SdcActorDev;      // sdc_actor.hpp

extern "C" {
// one env-step: sdc_step.hip (general; two envs per wavefront; four), sdc_wide.hip (one lane per env and its general form)
__global__ void sdc_dynamics_kernel(SdcDev S, int rel_hint, const int32_t* actions, float* obs, float* share_obs, unsigned char* done,
                                    float* info, float* final_obs, float* rew);
__global__ void sdc_dynamics_fast_kernel(SdcDev S, int rel_hint, const int32_t* actions, float* obs, float* share_obs, unsigned char* done,
                                         float* info, float* final_obs, float* rew);
__global__ void sdc_dynamics_quad_kernel(SdcDev S, int rel_hint, const int32_t* actions, float* obs, float* share_obs, unsigned char* done,
                                         float* info, float* final_obs, float* rew);
__global__ void sdc_dynamics_wide_kernel(SdcDev S, int rel_hint, const int32_t* actions, float* obs, float* share_obs, unsigned char* done,
                                         float* info, float* final_obs, float* rew);
__global__ void sdc_dynamics_wide_gen_kernel(SdcDev S, int rel_hint, const int32_t* actions, float* obs, float* share_obs,
                                             unsigned char* done, float* info, float* final_obs, float* rew);
// K env-steps: sdc_rollout.hip
__global__ void sdc_rollout_kernel(SdcDev S, int K, int rel_hint, const int32_t* actions, float* obs, float* share_obs, unsigned char* done,
                                   float* info, float* final_obs, float* rew);
__global__ void sdc_rollout_fast_kernel(SdcDev S, int K, int rel_hint, const int32_t* actions, float* obs, float* share_obs,
                                        unsigned char* done, float* info, float* final_obs, float* rew);
__global__ void sdc_rollout_quad_kernel(SdcDev S, int K, int rel_hint, const int32_t* actions, float* obs, float* share_obs,
                                        unsigned char* done, float* info, float* final_obs, float* rew);
// ... with the actors inside (the closed loop)
__global__ void sdc_rollout_actor_kernel(SdcDev S, int K, int rel_hint, const SdcActorDev* nets, const float* obs_in, int sample, float* obs,
                                         float* share_obs, unsigned char* done, float* info, float* final_obs, float* rew,
                                         int32_t* actions_out, float* logits_out, float* obs_latch);
__global__ void sdc_rollout_actor_quad_kernel(SdcDev S, int K, int rel_hint, const SdcActorDev* nets, const float* obs_in, int sample,
                                              float* obs, float* share_obs, unsigned char* done, float* info, float* final_obs, float* rew,
                                              int32_t* actions_out, float* logits_out, float* obs_latch);
// the episode boundary: sdc_reset.hip, sdc_features.hip
__global__ void sdc_reset_kernel(SdcDev S, int use_override, const int* ovr_day, const int* ovr_hour, const double* ovr_ci_min,
                                 const double* ovr_ci_max, const double* ovr_t_min, const double* ovr_t_max, int only_done, float* obs,
                                 float* share_obs, const double* inj_noise, const int* inj_roll);
__global__ void sdc_features_kernel(SdcDev S, int use_sma);
// verify mode: sdc_verify.hip
__global__ void sdc_reward_verify_kernel(SdcDev S, float* info);
}  // extern "C"

// the closed-loop kernels' dynamic LDS (sdc_rollout.hip)
size_t sdc_rollout_actor_lds_bytes();
size_t sdc_rollout_actor_quad_lds_bytes();
