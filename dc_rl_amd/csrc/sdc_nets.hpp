// sdc_nets.hpp -- A TRAINABLE NETWORK AS THE HANDLE HOLDS IT: one record, SdcNet, for each of the three actor slots and for the critic --
// the optimiser's master parameters, Adam's moments and state block, the packed copies the kernels read with their gather table, the
// partial-gradient buffer of the backward, and the three host facts a call asks of a network (its activation, whether its feature
// LayerNorm is on, whether it has been set).  sdc_capi.hip allocates one array per member for a kind's networks, sdc_nets_fill does the
// slot arithmetic ONCE (slot s of an array: base + s x the element size) and no later site repeats it; sdc_net_adam_plan derives the
// optimiser step's plan from a record.  What only the critic has (scale, shift and flags, the ValueNorm block, the value loss' and the
// ValueNorm's partial sums) stays beside its record in sdc_handle.
//
// Plain C++17: no HIP, no sdc_handle, no pointer followed -- a host compiler alone builds it (tests/test_host_nets.py fills the four
// records from made-up base addresses and holds every field and every plan to the public constants, plain and under the sanitizers).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/sustaindc_hip.h"
#include "sdc_optim_dev.hpp"      // SdcAdamStep, SDC_ADAM_MAX_PACKS: the HIP-free part

// which packed copy is which: an actor's SdcActorDev (the closed loop, sdc_actor.hpp), SdcActorEvalDev (stored rows,
// sdc_actor_eval_pack.hpp) and SdcActorGradDev (the transposes of the backward, sdc_actor_grad_pack.hpp); the critic's SdcCriticDev
// (sdc_critic_pack.hpp) and SdcCriticGradDev (sdc_critic_grad_pack.hpp)
enum { SDC_ACTOR_PACK_LOOP = 0, SDC_ACTOR_PACK_EVAL = 1, SDC_ACTOR_PACK_GRAD = 2, SDC_ACTOR_N_PACKS = 3 };
enum { SDC_CRITIC_PACK_VALUES = 0, SDC_CRITIC_PACK_GRAD = 1, SDC_CRITIC_N_PACKS = 2 };

// Every pointer is the device's and null until the first network of the kind is set (sdc_set_actor / sdc_set_critic allocate for all of
// the kind at once, and fill the one that is set).  The gather table (sdc_pack_tables.hpp) is uploaded once per kind and shared by its
// networks, and so is grad_part, allocated by the first backward: the workgroups' partial gradients [grad_max_blocks][n_params].
struct SdcNet {
  int n_params = 0;                            // SDC_ACTOR_N_PARAMS / SDC_CRITIC_N_PARAMS
  float *params = nullptr, *m = nullptr, *v = nullptr;      // [n_params] each: the fp32 master copy (the params struct's leading floats), Adam's moments
  sdc_optim_state* state = nullptr;            // [1]
  const int32_t* table = nullptr;              // the packs' tables behind each other; pack i's: table + table_offset[i]
  int table_offset[SDC_ADAM_MAX_PACKS + 1] = {};
  int n_packs = 0;
  uint32_t* pack[SDC_ADAM_MAX_PACKS] = {};     // this network's packed struct i ...
  int pack_dwords[SDC_ADAM_MAX_PACKS] = {};    // ... of sizeof / 4 dwords
  float* grad_part = nullptr;
  int grad_max_blocks = 0;                     // SDC_ACTOR_GRAD_MAX_BLOCKS / SDC_CRITIC_GRAD_MAX_BLOCKS
  int n_in = 0;                                // input width: SDC_ACT_IN / SDC_CRITIC_IN
  int activation = 0;                          // 0 tanh, 1 relu
  bool feature_norm = false;                   // the LayerNorm over the inputs is on
  bool set = false;

  // the optimiser leaves the leading elements alone where the feature LayerNorm is off: its gamma and beta, n_in each
  int first() const { return feature_norm ? 0 : 2 * n_in; }
  template <class DEV>
  DEV* pack_as(const int i) const { return reinterpret_cast<DEV*>(pack[i]); }
};

// a record of a kind of network before anything is allocated: its constants, and its packs' dwords from table_offset [n_packs + 1],
// SdcPackTables' (the table has one entry per dword of a packed struct)
inline SdcNet sdc_net_kind(const int n_params, const int n_in, const int grad_max_blocks, const int n_packs, const int* const table_offset) {
  SdcNet n;
  n.n_params = n_params, n.n_in = n_in, n.grad_max_blocks = grad_max_blocks, n.n_packs = n_packs;
  for (int i = 0; i <= n_packs; i++) n.table_offset[i] = table_offset[i];
  for (int i = 0; i < n_packs; i++) n.pack_dwords[i] = table_offset[i + 1] - table_offset[i];
  return n;
}

// the records of the `count` networks of one kind from `first`, slot 0's, whose pointers are the bases of arrays of `count` elements
// each (the one table but for): slot s's are base + s x the element size
inline void sdc_nets_fill(SdcNet* const nets, const int count, const SdcNet& first) {
  for (int s = 0; s < count; s++) {
    SdcNet& n = nets[s] = first;
    n.params += (size_t)s * n.n_params, n.m += (size_t)s * n.n_params, n.v += (size_t)s * n.n_params;
    n.state += s;
    for (int i = 0; i < n.n_packs; i++) n.pack[i] += (size_t)s * n.pack_dwords[i];
  }
}

// one optimiser step of a network: sdc_actor_adam_step's and sdc_critic_adam_step's plan
inline SdcAdamStep sdc_net_adam_plan(const SdcNet& n, const float* grads, const sdc_adam& adam, double* grad_norm) {
  SdcAdamStep P{grads, n.params, n.m, n.v, n.state, grad_norm, adam, n.n_params, n.first(), n.n_packs, n.table, {}, {}};
  for (int i = 0; i < n.n_packs; i++) P.pack[i] = n.pack[i], P.pack_dwords[i] = n.pack_dwords[i];
  return P;
}
