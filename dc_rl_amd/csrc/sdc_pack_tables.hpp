// sdc_pack_tables.hpp -- THE GATHER TABLES of the optimiser step: for every dword of a packed struct (an actor's SdcActorDev,
// SdcActorEvalDev and SdcActorGradDev, the critic's SdcCriticDev and SdcCriticGradDev) the index of the master parameter it holds, or
// SDC_PACK_CONST for a dword that holds none (padding, zeros beyond the inputs, flags, the critic's scale and shift).  The step
// (sdc_optim.hip) rewrites packed[d] = params[table[d]] for the others and leaves the constants as sdc_set_* wrote them.
//
// NO LAYOUT IS RESTATED HERE: a table is derived from the pack function itself.  The pack runs over a parameter struct whose floats
// hold their own index (6 459 < 2^24: every index is an exact float) and once more over one whose floats hold index + 8192; a dword
// that changed holds the parameter its first value names, a dword that did not is a constant.
//
// Plain C++17: no HIP, no sdc_handle -- a host compiler alone builds it (tests/test_optim_abi.py gathers random parameters through
// every table and holds the result to the pack's own bytes).
#pragma once

#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "sdc_actor_grad_pack.hpp"
#include "sdc_actor_pack.hpp"
#include "sdc_critic_grad_pack.hpp"

#define SDC_PACK_CONST (-1)

// the tables of one network behind each other: entry d of pack i is table[offset[i] + d]
template <int PACKS>
struct SdcPackTables {
  std::vector<int32_t> table;
  int offset[PACKS + 1] = {};      // in dwords; offset[PACKS]: the total
};

// PARAMS with its first n_floats floats holding base, base + 1, ...
template <class PARAMS>
inline void sdc_pack_fill_index(PARAMS* p, const int n_floats, const float base) {
  float* const f = reinterpret_cast<float*>(p);
  for (int j = 0; j < n_floats; j++) f[j] = base + (float)j;
}

// one pack's table appended to `out`: `pack(params, dev)` is the host pack
template <class DEV, class PARAMS, class PACK>
inline void sdc_pack_table_append(const PARAMS& p0, const PARAMS& p1, PACK pack, std::vector<int32_t>& out) {
  static_assert(sizeof(DEV) % 4 == 0, "dwords");
  std::unique_ptr<DEV> a(new DEV), b(new DEV);
  std::memset(a.get(), 0, sizeof(DEV));
  std::memset(b.get(), 0, sizeof(DEV));
  pack(&p0, a.get());
  pack(&p1, b.get());
  const size_t n = sizeof(DEV) / 4;
  for (size_t d = 0; d < n; d++) {
    uint32_t x, y;
    float f;
    std::memcpy(&x, reinterpret_cast<const unsigned char*>(a.get()) + 4 * d, 4);
    std::memcpy(&y, reinterpret_cast<const unsigned char*>(b.get()) + 4 * d, 4);
    std::memcpy(&f, &x, 4);
    out.push_back(x == y ? SDC_PACK_CONST : (int32_t)f);
  }
}

// an actor's three packed copies: SdcActorDev, SdcActorEvalDev, SdcActorGradDev (any flags: no parameter's place depends on them)
inline SdcPackTables<3> sdc_actor_pack_tables() {
  std::unique_ptr<sdc_actor_params> p0(new sdc_actor_params()), p1(new sdc_actor_params());
  sdc_pack_fill_index(p0.get(), SDC_ACTOR_N_PARAMS, 0.0f);
  sdc_pack_fill_index(p1.get(), SDC_ACTOR_N_PARAMS, 8192.0f);
  SdcPackTables<3> t;
  sdc_pack_table_append<SdcActorDev>(*p0, *p1, sdc_actor_pack, t.table);
  t.offset[1] = (int)t.table.size();
  sdc_pack_table_append<SdcActorEvalDev>(*p0, *p1, sdc_actor_eval_pack, t.table);
  t.offset[2] = (int)t.table.size();
  sdc_pack_table_append<SdcActorGradDev>(*p0, *p1, sdc_actor_grad_pack, t.table);
  t.offset[3] = (int)t.table.size();
  return t;
}

// the critic's two: SdcCriticDev, SdcCriticGradDev (scale, shift and flags are the same in both runs: constants)
inline SdcPackTables<2> sdc_critic_pack_tables() {
  std::unique_ptr<sdc_critic_params> p0(new sdc_critic_params()), p1(new sdc_critic_params());
  sdc_pack_fill_index(p0.get(), SDC_CRITIC_N_PARAMS, 0.0f);
  sdc_pack_fill_index(p1.get(), SDC_CRITIC_N_PARAMS, 8192.0f);
  p0->scale = p1->scale = 1.0f;
  SdcPackTables<2> t;
  sdc_pack_table_append<SdcCriticDev>(*p0, *p1, sdc_critic_pack, t.table);
  t.offset[1] = (int)t.table.size();
  sdc_pack_table_append<SdcCriticGradDev>(*p0, *p1, sdc_critic_grad_pack, t.table);
  t.offset[2] = (int)t.table.size();
  return t;
}

// the master parameters' place in the params structs: their first SDC_*_N_PARAMS floats, in declaration order
static_assert(offsetof(sdc_actor_params, ln0_gamma) == 0 && offsetof(sdc_critic_params, ln0_g) == 0, "the params lead their structs");
