"""A trainable network as the handle holds it (csrc/sdc_nets.hpp), without a GPU: the header compiled by g++ alone into a program that
fills the four records -- three actor slots, the critic -- from made-up, distinct base addresses (never followed) the way sdc_capi.hip
does, and prints every field of each record and of the optimiser step's plan derived from it, with the feature LayerNorm on and off.
Held to values written out here from the public constants: 6391 and 6459 parameters, inputs 26 and 29 wide, sizeof / 4 of the five
packed structs, the offsets sdc_actor_pack_tables() / sdc_critic_pack_tables() return --
  slot s's pointers are base + s x the element size, the table is the kind's one table, `first` is 0 or twice the input width, n_packs
  is 3 and 2, no two networks' ranges overlap and each lies inside its allocation, and the plan hands on exactly the record's own.
The same program runs built with -fsanitize=address,undefined (a stand-alone executable: nothing is loaded into Python)."""
import itertools
import subprocess

import pytest

from dc_rl_amd import _lib as L

DRIVER = r"""
#include <cstdio>
#include "sdc_nets.hpp"
#include "sdc_pack_tables.hpp"

template <class T>
static T* at(const unsigned long long a) { return reinterpret_cast<T*>((uintptr_t)a); }
static unsigned long long u(const void* p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

static void print(const char* name, const int ln, const SdcNet& n) {
  std::printf("net %s ln %d n_params %d params %llu m %llu v %llu state %llu table %llu n_packs %d grad_part %llu grad_max_blocks %d n_in %d "
              "activation %d feature_norm %d set %d first %d",
              name, ln, n.n_params, u(n.params), u(n.m), u(n.v), u(n.state), u(n.table), n.n_packs, u(n.grad_part), n.grad_max_blocks, n.n_in,
              n.activation, (int)n.feature_norm, (int)n.set, n.first());
  for (int i = 0; i <= SDC_ADAM_MAX_PACKS; i++) std::printf(" offset%d %d", i, n.table_offset[i]);
  for (int i = 0; i < SDC_ADAM_MAX_PACKS; i++) std::printf(" pack%d %llu dwords%d %d", i, u(n.pack[i]), i, n.pack_dwords[i]);
  std::printf("\n");
  const sdc_adam adam{5e-4, 0.9, 0.999, 1e-5, 0.01, 10.0};
  const SdcAdamStep P = sdc_net_adam_plan(n, at<const float>(0x7100000000ull), adam, at<double>(0x7200000000ull));
  std::printf("plan %s ln %d grads %llu params %llu m %llu v %llu state %llu grad_norm %llu lr %a beta1 %a beta2 %a eps %a weight_decay %a "
              "max_grad_norm %a n %d first %d n_packs %d table %llu",
              name, ln, u(P.grads), u(P.params), u(P.m), u(P.v), u(P.state), u(P.grad_norm), P.adam.lr, P.adam.beta1, P.adam.beta2, P.adam.eps,
              P.adam.weight_decay, P.adam.max_grad_norm, P.n, P.first, P.n_packs, u(P.table));
  for (int i = 0; i < SDC_ADAM_MAX_PACKS; i++) std::printf(" pack%d %llu dwords%d %d", i, u(P.pack[i]), i, P.pack_dwords[i]);
  std::printf("\n");
}

// slot 0's record of a kind with the arrays' bases: `k` picks the high digits, the arrays lie 2^32 apart
static SdcNet bases(SdcNet b, const unsigned long long k) {
  b.params = at<float>(k + 0x100000000ull), b.m = at<float>(k + 0x200000000ull), b.v = at<float>(k + 0x300000000ull);
  b.state = at<sdc_optim_state>(k + 0x400000000ull), b.table = at<const int32_t>(k + 0x500000000ull);
  for (int i = 0; i < b.n_packs; i++) b.pack[i] = at<uint32_t>(k + 0x600000000ull + i * 0x100000000ull);
  return b;
}

int main() {
  const SdcPackTables<3> ta = sdc_actor_pack_tables();
  const SdcPackTables<2> tc = sdc_critic_pack_tables();
  std::printf("sizes SdcActorDev %zu SdcActorEvalDev %zu SdcActorGradDev %zu SdcCriticDev %zu SdcCriticGradDev %zu sdc_optim_state %zu\n",
              sizeof(SdcActorDev), sizeof(SdcActorEvalDev), sizeof(SdcActorGradDev), sizeof(SdcCriticDev), sizeof(SdcCriticGradDev),
              sizeof(sdc_optim_state));
  std::printf("tables actor %d %d %d %d critic %d %d %d entries %zu %zu\n", ta.offset[0], ta.offset[1], ta.offset[2], ta.offset[3], tc.offset[0],
              tc.offset[1], tc.offset[2], ta.table.size(), tc.table.size());
  static const char* const names[4] = {"actor0", "actor1", "actor2", "critic"};
  for (int ln = 0; ln < 2; ln++) {
    SdcNet actor[3], critic;
    sdc_nets_fill(actor, 3, bases(sdc_net_kind(SDC_ACTOR_N_PARAMS, SDC_ACT_IN, SDC_ACTOR_GRAD_MAX_BLOCKS, SDC_ACTOR_N_PACKS, ta.offset), 0x1000000000ull));
    sdc_nets_fill(&critic, 1, bases(sdc_net_kind(SDC_CRITIC_N_PARAMS, SDC_CRITIC_IN, SDC_CRITIC_GRAD_MAX_BLOCKS, SDC_CRITIC_N_PACKS, tc.offset), 0x2000000000ull));
    if (ln == 0)
      for (int s = 0; s < 4; s++) print(names[s], -1, s < 3 ? actor[s] : critic);      // as filled: nothing set yet
    for (int s = 0; s < 4; s++) {      // as a set and a first backward leave them
      SdcNet& n = s < 3 ? actor[s] : critic;
      n.set = true, n.activation = (s + ln) & 1, n.feature_norm = ln != 0;
      n.grad_part = at<float>(s < 3 ? 0x1900000000ull : 0x2900000000ull);
      print(names[s], ln, n);
    }
  }
  return 0;
}
"""

ACTOR_BASE, CRITIC_BASE, GB4 = 0x1000000000, 0x2000000000, 0x100000000
GRADS, GRAD_NORM = 0x7100000000, 0x7200000000
# bytes of the packed structs where a test of the project already states them (tests/test_optim_abi.py, csrc/sdc_critic_pack.hpp)
KNOWN_BYTES = {"SdcActorEvalDev": 26144, "SdcActorGradDev": 16 * 64 * 6 * 4, "SdcCriticDev": 26640, "SdcCriticGradDev": 16 * 64 * 6 * 4,
               "sdc_optim_state": 32}
ADAM = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-5, weight_decay=0.01, max_grad_norm=10.0)


def build(td, flags, name):
    src = td / "nets.cpp"
    src.write_text(DRIVER)
    exe = str(td / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + L.CSRC, str(src)] + flags + ["-o", exe], check=True)
    return exe


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
    return r.stdout


def parse(text):
    """-> (sizes, tables, {(kind, name, ln): fields})"""
    lines = [ln.split() for ln in text.splitlines()]
    pairs = lambda w: dict(zip(w[0::2], w[1::2]))
    sizes = {k: int(v) for k, v in pairs(lines[0][1:]).items()}
    t = lines[1]
    tables = {"actor": [int(x) for x in t[2:6]], "critic": [int(x) for x in t[7:10]], "entries": [int(x) for x in t[11:13]]}
    recs = {}
    for w in lines[2:]:
        f = pairs(w[2:])
        key = (w[0], w[1], int(f.pop("ln")))
        assert key not in recs
        recs[key] = {k: (float.fromhex(v) if v.startswith(("0x", "-0x")) else int(v)) for k, v in f.items()}
    return sizes, tables, recs


def expected_net(name, ln, sizes, tables):
    """the record of network `name` written out from the constants; ln -1: as filled, 0 / 1: set with the feature LayerNorm off / on"""
    actor = name != "critic"
    s = int(name[-1]) if actor else 0
    base = ACTOR_BASE if actor else CRITIC_BASE
    n_params, n_in, n_packs = (6391, 26, 3) if actor else (6459, 29, 2)
    structs = ["SdcActorDev", "SdcActorEvalDev", "SdcActorGradDev"] if actor else ["SdcCriticDev", "SdcCriticGradDev"]
    dwords = [sizes[x] // 4 for x in structs] + [0] * (3 - n_packs)
    offsets = list(itertools.accumulate([0] + dwords[:n_packs])) + [0] * (3 - n_packs)
    assert offsets[:n_packs + 1] == tables["actor" if actor else "critic"]      # (one table entry per dword of a packed struct)
    slot = 3 if not actor else s
    want = dict(n_params=n_params, params=base + GB4 + s * 4 * n_params, m=base + 2 * GB4 + s * 4 * n_params, v=base + 3 * GB4 + s * 4 * n_params,
                state=base + 4 * GB4 + s * sizes["sdc_optim_state"], table=base + 5 * GB4, n_packs=n_packs, grad_max_blocks=256, n_in=n_in,
                grad_part=0 if ln < 0 else base + 9 * GB4, activation=0 if ln < 0 else (slot + ln) & 1, feature_norm=int(ln > 0), set=int(ln >= 0),
                first=0 if ln > 0 else 2 * n_in)
    for i in range(4):
        want["offset%d" % i] = offsets[i]
    for i in range(3):
        want["pack%d" % i] = base + (6 + i) * GB4 + s * 4 * dwords[i] if i < n_packs else 0
        want["dwords%d" % i] = dwords[i]
    return want


def expected_plan(net):
    want = dict(grads=GRADS, grad_norm=GRAD_NORM, n=net["n_params"], **ADAM)
    for k in ["params", "m", "v", "state", "first", "n_packs", "table"] + ["pack%d" % i for i in range(3)] + ["dwords%d" % i for i in range(3)]:
        want[k] = net[k]
    return want


def ranges(net, sizes):
    """every array that is one network's own, as [start, end) in bytes"""
    out = [(net[k], net[k] + 4 * net["n_params"]) for k in ("params", "m", "v")]
    out.append((net["state"], net["state"] + sizes["sdc_optim_state"]))
    out += [(net["pack%d" % i], net["pack%d" % i] + 4 * net["dwords%d" % i]) for i in range(net["n_packs"])]
    return out


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return run(build(tmp_path_factory.mktemp("nets"), ["-O1"], "nets"))


def test_header_is_hip_free():
    src = open(L.CSRC + "/sdc_nets.hpp").read()
    assert "hip_runtime" not in src and "hipStream" not in src and "hipError" not in src and "sdc_handle" not in src.split("#pragma once")[1]
    dev = open(L.CSRC + "/sdc_optim_dev.hpp").read()      # (the plan's struct stands once, in the part of its header that holds no HIP)
    assert "hip" not in dev.split("#pragma once")[1].split("#if defined(__HIPCC__)")[0] and "struct SdcAdamStep {" in dev


def test_records_and_plans_equal_the_constants(plain):
    sizes, tables, recs = parse(plain)
    assert {k: sizes[k] for k in KNOWN_BYTES} == KNOWN_BYTES and all(v % 4 == 0 for v in sizes.values())
    assert (L.ACTOR_N_PARAMS, L.CRITIC_N_PARAMS) == (6391, 6459) and tables["entries"] == [tables["actor"][3], tables["critic"][2]]
    names = ["actor0", "actor1", "actor2", "critic"]
    assert set(recs) == {(kind, n, ln) for kind in ("net", "plan") for n in names for ln in (-1, 0, 1)}
    for n in names:
        for ln in (-1, 0, 1):
            want = expected_net(n, ln, sizes, tables)
            assert recs[("net", n, ln)] == want, (n, ln, {k: (recs[("net", n, ln)].get(k), want[k]) for k in want if recs[("net", n, ln)].get(k) != want[k]})
            assert recs[("plan", n, ln)] == expected_plan(want), (n, ln)
    # what the figures above amount to, said outright
    for ln in (0, 1):
        assert [recs[("net", n, ln)]["first"] for n in names] == ([0, 0, 0, 0] if ln else [52, 52, 52, 58])
        assert [recs[("net", n, ln)]["n_packs"] for n in names] == [3, 3, 3, 2]
        assert len({recs[("net", n, ln)]["table"] for n in names[:3]}) == 1 and recs[("net", "critic", ln)]["table"] != recs[("net", "actor0", ln)]["table"]
        assert recs[("plan", "critic", ln)]["pack2"] == 0 and recs[("plan", "critic", ln)]["dwords2"] == 0


def test_no_two_networks_overlap_and_each_lies_inside_its_allocation(plain):
    sizes, _, recs = parse(plain)
    nets = {n: recs[("net", n, 1)] for n in ("actor0", "actor1", "actor2", "critic")}
    spans = [(n, a, b) for n, net in nets.items() for a, b in ranges(net, sizes)]
    assert len(spans) == 3 * 7 + 6 and all(a < b for _, a, b in spans)
    for (n1, a1, b1), (n2, a2, b2) in itertools.combinations(spans, 2):
        assert b1 <= a2 or b2 <= a1, (n1, n2, a1, b1, a2, b2)
    # an allocation holds `count` elements from its base: the last slot ends where it ends
    for n, net in nets.items():
        count, base = (3, ACTOR_BASE) if n != "critic" else (1, CRITIC_BASE)
        for j, (a, b) in enumerate(ranges(net, sizes)):
            start = base + (j + 1) * GB4 if j < 4 else base + (6 + j - 4) * GB4
            assert start <= a and b <= start + count * (b - a), (n, j)
    last = ranges(nets["actor2"], sizes)
    assert [b - (ACTOR_BASE + (j + 1) * GB4) for j, (_, b) in enumerate(last[:3])] == [3 * 4 * 6391] * 3


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    """a stand-alone program run on its own: nothing is loaded into Python"""
    san = build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "nets_san")
    assert run(san) == plain
