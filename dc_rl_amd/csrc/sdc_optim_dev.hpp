// sdc_optim_dev.hpp -- the launch plans of sdc_optim.hip: sdc_adam_update_kernel and sdc_adam_gather_kernel (sdc_actor_adam_step /
// sdc_critic_adam_step) and sdc_critic_norm_kernel (sdc_set_critic_norm).  The arithmetic: sdc_optim.hpp; the gather tables:
// sdc_pack_tables.hpp; the contract: include/sustaindc_hip.h THE OPTIMISER STEP.
//
// THE PLAN: this is latency-bound work on ~6.4 K parameters and ~19.3 K packed dwords, two small launches on the call's stream.
// sdc_adam_update_kernel, ONE workgroup of SDC_ADAM_BLOCK lanes (the sum of squares has one fixed order):
//   1. lanes 0 .. 255 form the sum of squares in sdc_actor_grad_sq_kernel's order (sdc_adam_lane_sq, then the tree from 128 down);
//   2. lane 0 reads the state block, writes grad_norm, prepares the scalars (sdc_adam_prepare) into LDS and writes the state back;
//   3. behind a barrier every lane steps the elements j = first + l, first + l + SDC_ADAM_BLOCK, ... < n (sdc_adam_element): an element
//      is read and written by one lane only.  A skipped step (S not finite) ends after 2.
// sdc_adam_gather_kernel, SDC_ADAM_GATHER_BLOCKS workgroups behind it on the stream: lane l of workgroup b rewrites the packed dwords
// d = b * SDC_ADAM_BLOCK + l, + the grid's lanes, ... of every packed copy: packed[d] = params[table[d]] unless table[d] is
// SDC_PACK_CONST.  It does not ask whether the step was skipped: it then rewrites every dword with the bits it already holds.
// ADDRESS BOUNDS: j < n = the length of grads / params / m / v; table entries are < n by construction (sdc_pack_tables.hpp: the indices
// the pack itself placed) and d < pack_dwords[i] = sizeof of the packed struct / 4; every buffer is the handle's but grads.
// Built with -DSDC_OPTIM_ONE_LAUNCH the same body runs as ONE launch of one workgroup with a barrier between update and gather
// (sdc_adam_step_kernel): the form this one was measured against with tools/update_rate.py and found 0.010 ms slower per step
// (DESIGN.md section 4.31).
//
// THE PLANS ARE PLAIN TYPES: up to the launchers this header holds no HIP, and a host compiler alone builds it (sdc_nets.hpp derives
// SdcAdamStep from a network's record; tests/test_host_nets.py holds that without a GPU).
#pragma once

#include <cstdint>

#include "sdc_critic_pack.hpp"
#include "sdc_optim.hpp"

#define SDC_ADAM_BLOCK 1024
#define SDC_ADAM_MAX_PACKS 3
#define SDC_ADAM_GATHER_BLOCKS 20

struct SdcAdamStep {
  const float* grads;            // [n]
  float* params;                 // [n] the master copy
  float* m;                      // [n]
  float* v;                      // [n]
  sdc_optim_state* state;        // [1]
  double* grad_norm;             // [1] or NULL
  sdc_adam adam;
  int n;                         // SDC_ACTOR_N_PARAMS / SDC_CRITIC_N_PARAMS
  int first;                     // leading elements left alone (feature LayerNorm off: its ln0 entries)
  int n_packs;
  const int32_t* table;          // the packs' gather tables behind each other
  uint32_t* pack[SDC_ADAM_MAX_PACKS];
  int pack_dwords[SDC_ADAM_MAX_PACKS];
};

struct SdcCriticNorm {
  SdcCriticDev* critic;
  float scale, shift;
};

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

hipError_t sdc_adam_step_launch(const SdcAdamStep& P, hipStream_t st);
hipError_t sdc_critic_norm_launch(const SdcCriticNorm& P, hipStream_t st);
#endif
