"""The optimiser step on the CPU side (include/sustaindc_hip.h THE OPTIMISER STEP): the nine entry points declared, exported and bound
with the ABI still at 313 and their two structs mirrored; a null handle refused before any device work; sdc_optim.hip cross-compiles for
gfx950 with no scratch and no spills for exactly its kernels; and three stand-alone programs built by the host compiler alone with
-ffp-contract=off, plain and with -fsanitize=address,undefined (nothing is loaded into Python):
  (a) csrc/sdc_optim.hpp's step over the cases of tests/test_optim_ref.py equals the NumPy restatement tests/optim_ref.py bit for bit:
      p, m, v, the state block and the norm after every step;
  (b) for random parameters, gathering through each of the five tables of csrc/sdc_pack_tables.hpp gives the host pack's bytes exactly,
      every parameter a pack holds is placed exactly once, and every "constant" dword is zero padding or a flag / scale / shift member;
  (c) every text the new calls refuse with (csrc/sdc_refusals.hpp): one request line per case in, the rule's message or `-` out.

A request line of (c):  <entry point> key=value ...   Defaults: a handle with all three actors and a critic set, agent_slot 0, every
array at a made-up 4096-byte aligned address (a number, 0: NULL, never followed) but m, v and the state of the set_*_optim calls, which
are the program's own (clean ones; `bad_m` / `bad_v` plant a value), lr 5e-4, betas 0.9 / 0.999, eps 1e-5, weight_decay 0,
max_grad_norm 10."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import optim_ref as O
from tests.plan_util import assert_c_layout, assert_no_scratch_or_spills, entry_point_header, kernel_resources

ENTRY_POINTS = {
    "sdc_actor_adam_step": ["h", "agent_slot", "grads", "adam", "grad_norm", "stream"],
    "sdc_critic_adam_step": ["h", "grads", "adam", "grad_norm", "stream"],
    "sdc_get_actor": ["h", "agent_slot", "out"],
    "sdc_get_critic": ["h", "out"],
    "sdc_get_actor_optim": ["h", "agent_slot", "m", "v", "st"],
    "sdc_set_actor_optim": ["h", "agent_slot", "m", "v", "st"],
    "sdc_get_critic_optim": ["h", "m", "v", "st"],
    "sdc_set_critic_optim": ["h", "m", "v", "st"],
    "sdc_set_critic_norm": ["h", "scale", "shift", "stream"],
}
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
CXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + L.CSRC]


def test_entry_points_are_declared_exported_and_bound_at_abi_313(tmp_path):
    for fn, args in ENTRY_POINTS.items():
        entry_point_header(fn, args, "sdc_optim.hip")
    assert_c_layout(tmp_path, "sdc_adam", L.SdcAdam, ["lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm"])
    assert_c_layout(tmp_path, "sdc_optim_state", L.SdcOptimState, ["step", "beta1_pow", "beta2_pow", "skipped"])
    hpp = open(os.path.join(L.CSRC, "sdc_optim.hpp")).read()
    assert "#define SDC_ADAM_SQ_LANES %d " % O.SQ_LANES in hpp
    for name in ("sdc_optim.hpp", "sdc_pack_tables.hpp", "sdc_actor_pack.hpp"):      # (HIP-free but for the markers)
        src = open(os.path.join(L.CSRC, name)).read()
        assert "hip_runtime" not in src and "hipStream" not in src and "sdc_handle" not in src.split("#pragma once")[1], name


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    adam = L.SdcAdam(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-5, weight_decay=0.0, max_grad_norm=10.0)
    import ctypes as C
    calls = {
        "sdc_actor_adam_step": lambda: lib.sdc_actor_adam_step(None, 0, None, C.byref(adam), None, None),
        "sdc_critic_adam_step": lambda: lib.sdc_critic_adam_step(None, None, C.byref(adam), None, None),
        "sdc_get_actor": lambda: lib.sdc_get_actor(None, 0, None),
        "sdc_get_critic": lambda: lib.sdc_get_critic(None, None),
        "sdc_get_actor_optim": lambda: lib.sdc_get_actor_optim(None, 0, None, None, None),
        "sdc_set_actor_optim": lambda: lib.sdc_set_actor_optim(None, 0, None, None, None),
        "sdc_get_critic_optim": lambda: lib.sdc_get_critic_optim(None, None, None, None),
        "sdc_set_critic_optim": lambda: lib.sdc_set_critic_optim(None, None, None, None),
        "sdc_set_critic_norm": lambda: lib.sdc_set_critic_norm(None, 1.0, 0.0, None),
    }
    assert set(calls) == set(ENTRY_POINTS)
    for fn, call in calls.items():
        assert call() == -2 and lib.sdc_last_error() == (fn + ": null handle").encode(), fn


def test_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_optim.hip")
    assert_no_scratch_or_spills(per, {"sdc_adam_update_kernel", "sdc_adam_gather_kernel", "sdc_critic_norm_kernel"})      # (two launches per step)
    for k, u in per.items():      # (recorded in DESIGN.md section 4.31, not gated)
        print(k, "VGPRs", u.get("VGPRs"), "SGPRs", u.get("TotalSGPRs"), "occupancy", u.get("Occupancy"), "LDS", u.get("LDS Size"))
    src = open(os.path.join(L.CSRC, "sdc_optim.hip")).read()
    assert "atomic" not in src.lower() and "#pragma clang fp contract(off)" in src


def build(td, text, flags, name):
    src = td / (name + ".cpp")
    src.write_text(text)
    exe = str(td / name)
    subprocess.run(CXX + [str(src)] + flags + ["-o", exe], check=True)
    return exe


# ---- (a) the header's step against the restatement ---------------------------------------------------------------------------------------
STEP_MAIN = r"""
#include <cstdio>
#include <vector>
#include "sdc_optim.hpp"
// in: int32 n, first, steps; sdc_adam; p, m, v [n]; steps x g [n].  out, per step: p, m, v [n], sdc_optim_state, double norm
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  int32_t hd[4];
  sdc_adam a;
  if (!f || std::fread(hd, 4, 4, f) != 4 || std::fread(&a, sizeof(a), 1, f) != 1) return 2;
  const int n = hd[0], first = hd[1], steps = hd[2];
  std::vector<float> p(n), m(n), v(n), g(n);
  if (std::fread(p.data(), 4, n, f) != (size_t)n || std::fread(m.data(), 4, n, f) != (size_t)n || std::fread(v.data(), 4, n, f) != (size_t)n) return 2;
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  sdc_optim_state st{0, 1.0, 1.0, 0};
  for (int s = 0; s < steps; s++) {
    if (std::fread(g.data(), 4, n, f) != (size_t)n) return 2;
    const double norm = sdc_adam_step_host(a, g.data(), n, first, p.data(), m.data(), v.data(), st);
    std::fwrite(p.data(), 4, n, o);
    std::fwrite(m.data(), 4, n, o);
    std::fwrite(v.data(), 4, n, o);
    std::fwrite(&st, sizeof(st), 1, o);
    std::fwrite(&norm, 8, 1, o);
  }
  std::fclose(f);
  std::fclose(o);
  return 0;
}
"""


@pytest.fixture(scope="module")
def step_programs(tmp_path_factory):
    td = tmp_path_factory.mktemp("optim_step")
    return td, [build(td, STEP_MAIN, ["-O2"], "step"), build(td, STEP_MAIN, SAN, "step_san")]


def run_steps(td, exe, grads, p0, m0, v0, first, lr, betas, eps, wd, clip):
    n = p0.size
    fin, fout = td / "in.bin", td / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<4i", n, first, len(grads), 0))
        f.write(struct.pack("<6d", lr, betas[0], betas[1], eps, wd, math.inf if clip is None else clip))
        for a in (p0, m0, v0, *grads):
            f.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
    raw, out, at = fout.read_bytes(), [], 0
    for _ in grads:
        arrays = [np.frombuffer(raw, np.float32, n, at + 4 * n * i) for i in range(3)]
        at += 12 * n
        step, b1, b2, skipped, norm = struct.unpack_from("<qddqd", raw, at)
        at += 40
        out.append((arrays, dict(step=step, beta1_pow=b1, beta2_pow=b2, skipped=skipped), norm))
    assert at == len(raw)
    return out


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def hold_to_restatement(td, exes, grads, p0, first, lr, betas, eps, wd, clip):
    z = np.zeros_like(p0)
    p, m, v, st = p0.copy(), z.copy(), z.copy(), O.new_state()
    want = []
    for g in grads:
        p, m, v, norm = O.step(g, p, m, v, st, lr, betas, eps, wd, clip, first=first)
        want.append(((p, m, v), dict(st), norm))
    for exe in exes:
        got = run_steps(td, exe, grads, p0, z, z, first, lr, betas, eps, wd, clip)
        for s, ((ga, gst, gnorm), (wa, wst, wnorm)) in enumerate(zip(got, want)):
            assert all(same_bits(x, y) for x, y in zip(ga, wa)), (exe, s)
            assert gst == wst, (exe, s, gst, wst)
            assert struct.pack("<d", gnorm) == struct.pack("<d", wnorm), (exe, s, gnorm, wnorm)
    return want


@pytest.mark.parametrize("clip", ["active", "inactive", "off"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_header_step_equals_the_restatement_bit_for_bit(step_programs, wd, clip):
    from tests.test_optim_ref import BETAS, CLIPS, EPS, LR, inputs
    td, exes = step_programs
    p0, grads = inputs()
    want = hold_to_restatement(td, exes, grads, p0, 0, LR, BETAS, EPS, wd, CLIPS[clip])
    assert want[-1][1]["step"] == len(grads)


def test_header_step_exact_cases(step_programs):
    from tests.test_optim_ref import BETAS, EPS, LR, N, inputs
    td, exes = step_programs
    p0, grads = inputs()
    # a zero gradient on zero moments leaves p; then a NaN and an infinity are skipped; then clean steps go on
    bad1, bad2 = grads[1].copy(), grads[2].copy()
    bad1[17] = np.nan
    bad2[N - 1] = -np.inf
    seq = [np.zeros(N, np.float32), grads[0], bad1, bad2, grads[3], grads[4]]
    want = hold_to_restatement(td, exes, seq[:2], p0, 0, LR, BETAS, EPS, 0.0, 10.0)
    assert same_bits(want[0][0][0], p0) and want[0][1]["step"] == 1 and not same_bits(want[1][0][0], p0)
    want = hold_to_restatement(td, exes, seq, p0, 0, LR, BETAS, EPS, 0.01, 10.0)
    assert [w[1]["skipped"] for w in want] == [0, 0, 1, 2, 2, 2] and [w[1]["step"] for w in want] == [1, 2, 2, 2, 3, 4]
    assert all(same_bits(x, y) for x, y in zip(want[3][0], want[1][0]))
    # the feature LayerNorm off: its 52 / 58 ln0 entries are left alone under weight decay
    for first in (52, 58):
        g = [x.copy() for x in grads[:3]]
        for x in g:
            x[:first] = 0.0
        want = hold_to_restatement(td, exes, g, p0, first, LR, BETAS, EPS, 0.01, 10.0)
        assert same_bits(want[-1][0][0][:first], p0[:first]) and not want[-1][0][1][:first].any()


# ---- (b) the gather tables against the packs' own bytes ------------------------------------------------------------------------------------
TABLE_MAIN = r"""
#include <cstdio>
#include <cstddef>
#include <memory>
#include <vector>
#include "sdc_pack_tables.hpp"

// one pack: gather through its table over a zeroed struct that holds the pack's constants, against the pack's own bytes
template <class DEV>
static void hold(const char* name, const int32_t* table, const int n_table, const float* params, const int n_params, const DEV& packed,
                 const int want_placed) {
  const int n = (int)(sizeof(DEV) / 4);
  const uint32_t* const src = reinterpret_cast<const uint32_t*>(params);
  const uint32_t* const want = reinterpret_cast<const uint32_t*>(&packed);
  std::vector<int> used(n_params, 0);
  int bad = 0, consts = 0, out_of_range = 0;
  std::printf("%s dwords %d table %d", name, n, n_table);
  std::vector<int> nonzero;
  for (int d = 0; d < n && d < n_table; d++) {
    const int32_t t = table[d];
    if (t == SDC_PACK_CONST) {
      consts++;
      if (want[d] != 0u) nonzero.push_back(4 * d);
      continue;
    }
    if (t < 0 || t >= n_params) { out_of_range++; continue; }
    used[t]++;
    if (src[t] != want[d]) bad++;
  }
  int once = 0, never = 0, more = 0;
  for (int j = 0; j < n_params; j++) (used[j] == 1 ? once : used[j] == 0 ? never : more)++;
  std::printf(" const %d mismatch %d out_of_range %d once %d never %d more %d want_placed %d nonzero_const", consts, bad, out_of_range,
              once, never, more, want_placed);
  for (int b : nonzero) std::printf(" %d", b);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::unique_ptr<sdc_actor_params> a(new sdc_actor_params);
  std::unique_ptr<sdc_critic_params> c(new sdc_critic_params);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(a.get(), sizeof(sdc_actor_params), 1, f) != 1) return 2;
  std::fclose(f);
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(c.get(), sizeof(sdc_critic_params), 1, f) != 1) return 2;
  std::fclose(f);
  const SdcPackTables<3> ta = sdc_actor_pack_tables();
  const SdcPackTables<2> tc = sdc_critic_pack_tables();
  std::unique_ptr<SdcActorDev> a0(new SdcActorDev);
  std::unique_ptr<SdcActorEvalDev> a1(new SdcActorEvalDev);
  std::unique_ptr<SdcActorGradDev> a2(new SdcActorGradDev);
  std::unique_ptr<SdcCriticDev> c0(new SdcCriticDev);
  std::unique_ptr<SdcCriticGradDev> c1(new SdcCriticGradDev);
  sdc_actor_pack(a.get(), a0.get());
  sdc_actor_eval_pack(a.get(), a1.get());
  sdc_actor_grad_pack(a.get(), a2.get());
  sdc_critic_pack(c.get(), c0.get());
  sdc_critic_grad_pack(c.get(), c1.get());
  const float* const pa = reinterpret_cast<const float*>(a.get());
  const float* const pc = reinterpret_cast<const float*>(c.get());
  std::printf("offsets actor_flags %zu eval_flags %zu critic_scale %zu critic_shift %zu critic_flags %zu actor_total %d critic_total %d\n",
              offsetof(SdcActorDev, flags), offsetof(SdcActorEvalDev, flags), offsetof(SdcCriticDev, scale), offsetof(SdcCriticDev, shift),
              offsetof(SdcCriticDev, flags), ta.offset[3], tc.offset[2]);
  hold("SdcActorDev", ta.table.data() + ta.offset[0], ta.offset[1] - ta.offset[0], pa, SDC_ACTOR_N_PARAMS, *a0, SDC_ACTOR_N_PARAMS);
  hold("SdcActorEvalDev", ta.table.data() + ta.offset[1], ta.offset[2] - ta.offset[1], pa, SDC_ACTOR_N_PARAMS, *a1, SDC_ACTOR_N_PARAMS);
  hold("SdcActorGradDev", ta.table.data() + ta.offset[2], ta.offset[3] - ta.offset[2], pa, SDC_ACTOR_N_PARAMS, *a2, 64 * 64 + 64 * 26);
  hold("SdcCriticDev", tc.table.data() + tc.offset[0], tc.offset[1] - tc.offset[0], pc, SDC_CRITIC_N_PARAMS, *c0, SDC_CRITIC_N_PARAMS);
  hold("SdcCriticGradDev", tc.table.data() + tc.offset[1], tc.offset[2] - tc.offset[1], pc, SDC_CRITIC_N_PARAMS, *c1, 64 * 64 + 64 * 29);
  return 0;
}
"""


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "sanitized"])
def test_gathering_through_the_tables_gives_the_packs_bytes(tmp_path, flags):
    exe = build(tmp_path, TABLE_MAIN, flags, "tables")
    rng = np.random.default_rng(5)
    a, c = L.SdcActorParams(), L.SdcCriticParams()
    # (every parameter its own non-zero value, in random order and of random sign: a swapped pair would show)
    draw = lambda n: ((rng.permutation(n) + 1) * rng.choice([-1.0, 1.0], n) * 2.0 ** -11 * 1.0009765625).astype(np.float32)
    va, vc = draw(L.ACTOR_N_PARAMS), draw(L.CRITIC_N_PARAMS)
    assert len(np.unique(va.view(np.uint32))) == va.size and len(np.unique(vc.view(np.uint32))) == vc.size and va.all() and vc.all()
    import ctypes as C
    C.memmove(C.byref(a), va.ctypes.data, va.nbytes)
    C.memmove(C.byref(c), vc.ctypes.data, vc.nbytes)
    a.use_feature_normalization, a.activation = 1, 1
    c.scale, c.shift, c.flags = 2.5, -1.25, 3
    (tmp_path / "a.bin").write_bytes(bytes(a))
    (tmp_path / "c.bin").write_bytes(bytes(c))
    r = subprocess.run([exe, str(tmp_path / "a.bin"), str(tmp_path / "c.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    off = dict(zip(lines[0].split()[1::2], map(int, lines[0].split()[2::2])))
    sizes = {"SdcActorDev": None, "SdcActorEvalDev": 26144, "SdcActorGradDev": 16 * 64 * 6 * 4, "SdcCriticDev": 26640,
             "SdcCriticGradDev": 16 * 64 * 6 * 4}
    flag_bytes = {"SdcActorDev": {off["actor_flags"]}, "SdcActorEvalDev": {off["eval_flags"]}, "SdcActorGradDev": set(),
                  "SdcCriticDev": {off["critic_scale"], off["critic_shift"], off["critic_flags"]}, "SdcCriticGradDev": set()}
    total = {"actor": 0, "critic": 0}
    assert [ln.split()[0] for ln in lines[1:]] == list(sizes)
    for ln in lines[1:]:
        w = ln.split()
        name, f = w[0], dict(zip(w[1:19:2], map(int, w[2:20:2])))
        nonzero = set(map(int, w[w.index("nonzero_const") + 1:]))
        assert f["dwords"] == f["table"] and (sizes[name] is None or 4 * f["dwords"] == sizes[name]), ln
        assert f["mismatch"] == 0 and f["out_of_range"] == 0 and f["more"] == 0, ln
        assert f["once"] == f["want_placed"] and f["const"] == f["dwords"] - f["want_placed"], ln
        # the parameters a transposed pack does not hold are all but w1 and w2
        assert f["never"] == (L.CRITIC_N_PARAMS if "Critic" in name else L.ACTOR_N_PARAMS) - f["want_placed"], ln
        assert nonzero == flag_bytes[name], ln      # (every other constant dword is zero padding)
        total["critic" if "Critic" in name else "actor"] += f["dwords"]
    assert total == {"actor": off["actor_total"], "critic": off["critic_total"]}


# ---- (c) the refusal texts -----------------------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <vector>
#include "sdc_refusals.hpp"

static std::map<std::string, std::string> R;
static const long long GOOD = 0x7f0000001000ll;
static long long I(const char* k, const long long dflt) { return R.count(k) ? std::strtoll(R[k].c_str(), nullptr, 0) : dflt; }
static double D(const char* k, const double dflt) { return R.count(k) ? std::strtod(R[k].c_str(), nullptr) : dflt; }
template <class T>
static T* P(const char* k, const long long dflt = GOOD) { return reinterpret_cast<T*>((uintptr_t)I(k, dflt)); }
static void out(const SdcMsg& m) { std::printf("%s\n", m ? m->c_str() : "-"); }

int main() {
  for (std::string line; std::getline(std::cin, line);) {
    std::stringstream ss(line);
    std::string entry, kv;
    ss >> entry;
    R.clear();
    while (ss >> kv) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) return 2;
      R[kv.substr(0, eq)] = kv.substr(eq + 1);
    }
    SdcCallFacts f;
    if (I("handle", 1)) {
      f.handle = true;
      f.n_envs = 8;
      f.critic_set = I("critic", 1) != 0;
      for (int a = 0; a < 3; a++) f.actor_set[a] = I("actors", 7) >> a & 1;
    }
    const bool actor = entry.find("actor") != std::string::npos;
    const int slot = actor ? (int)I("agent_slot", 0) : -1;
    sdc_adam adam{D("lr", 5e-4), D("beta1", 0.9), D("beta2", 0.999), D("eps", 1e-5), D("weight_decay", 0.0), D("max_grad_norm", 10.0)};
    if (entry == "sdc_actor_adam_step" || entry == "sdc_critic_adam_step") {
      out(sdc_adam_step_refused(entry.c_str(), f, actor, slot, P<float>("grads"), I("adam", 1) ? &adam : nullptr, P<double>("grad_norm")));
    } else if (entry == "sdc_get_actor" || entry == "sdc_get_critic" || entry == "sdc_get_actor_optim" || entry == "sdc_get_critic_optim") {
      out(sdc_optim_get_refused(entry.c_str(), f, actor, slot, I("out", 1) != 0));
    } else if (entry == "sdc_set_actor_optim" || entry == "sdc_set_critic_optim") {
      const int n = actor ? SDC_ACTOR_N_PARAMS : SDC_CRITIC_N_PARAMS;
      std::vector<float> m(n, 0.25f), v(n, 0.5f);
      if (R.count("bad_m")) m[n - 1] = (float)D("bad_m", 0.0);
      if (R.count("bad_v")) v[n / 2] = (float)D("bad_v", 0.0);
      sdc_optim_state st{I("step", 3), D("beta1_pow", 0.729), D("beta2_pow", 0.997), I("skipped", 1)};
      out(sdc_set_optim_refused(entry.c_str(), f, actor, slot, I("m", 1) ? m.data() : nullptr, I("v", 1) ? v.data() : nullptr,
                                I("st", 1) ? &st : nullptr));
    } else if (entry == "sdc_set_critic_norm") {
      out(sdc_set_critic_norm_refused(f, D("scale", 2.5), D("shift", -1.0)));
    } else {
      return 3;
    }
  }
  return 0;
}
"""

ODD, FOUR = 0x7f0000001002, 0x7f0000001004
ADAM_TEXTS = [
    ("lr=-1e-9", "lr must be finite and not negative"), ("lr=inf", "lr must be finite and not negative"), ("lr=nan", "lr must be finite and not negative"),
    ("beta1=1", "beta1 and beta2 must lie in [0, 1)"), ("beta1=-0.1", "beta1 and beta2 must lie in [0, 1)"), ("beta2=1.5", "beta1 and beta2 must lie in [0, 1)"),
    ("beta2=nan", "beta1 and beta2 must lie in [0, 1)"),
    ("eps=-1e-8", "eps must be finite and not negative"), ("eps=inf", "eps must be finite and not negative"),
    ("weight_decay=-0.01", "weight_decay must be finite and not negative"), ("weight_decay=nan", "weight_decay must be finite and not negative"),
    ("max_grad_norm=0", "max_grad_norm must be above 0 (+infinity: no clipping)"), ("max_grad_norm=-2", "max_grad_norm must be above 0 (+infinity: no clipping)"),
    ("max_grad_norm=nan", "max_grad_norm must be above 0 (+infinity: no clipping)"),
    ("adam=0", "null sdc_adam"),
]
STATE_TEXTS = [
    ("m=0", "null m, v or state"), ("v=0", "null m, v or state"), ("st=0", "null m, v or state"),
    ("step=-1", "step must not be negative"),
    ("beta1_pow=0", "beta1_pow and beta2_pow must lie in (0, 1]"), ("beta2_pow=1.0000001", "beta1_pow and beta2_pow must lie in (0, 1]"),
    ("beta1_pow=nan", "beta1_pow and beta2_pow must lie in (0, 1]"),
    ("skipped=-3", "skipped must not be negative"),
    ("bad_m=nan", "a moment that is not finite, or a negative v"), ("bad_v=inf", "a moment that is not finite, or a negative v"),
    ("bad_v=-1e-30", "a moment that is not finite, or a negative v"),
]
NO_ACTOR = "%s: no actor is set for agent_slot 1 (sdc_set_actor first)"
CASES = []
for fn in ("sdc_actor_adam_step", "sdc_critic_adam_step"):
    CASES += [(fn, None), (fn + " grad_norm=0 max_grad_norm=inf lr=0 eps=0 beta1=0 beta2=0 weight_decay=0.01", None), (fn + " grads=%d" % FOUR, None),
              (fn + " handle=0 grads=0", fn + ": null handle"),
              (fn + " grads=0", fn + ": null grads"), (fn + " grads=0 lr=-1", fn + ": null grads"),
              (fn + " grads=%d" % ODD, fn + ": grads not dword-aligned"),
              (fn + " grad_norm=%d" % FOUR, fn + ": grad_norm not 8-byte aligned"), (fn + " grad_norm=%d lr=nan" % ODD, fn + ": grad_norm not 8-byte aligned")]
    CASES += [("%s %s" % (fn, req), "%s: %s" % (fn, text)) for req, text in ADAM_TEXTS]
for fn in ("sdc_actor_adam_step", "sdc_get_actor", "sdc_get_actor_optim", "sdc_set_actor_optim"):
    CASES += [(fn + " agent_slot=2", None),
              (fn + " agent_slot=3", fn + ": agent_slot = 3 outside [0, 2]"), (fn + " agent_slot=-1 actors=0", fn + ": agent_slot = -1 outside [0, 2]"),
              (fn + " agent_slot=1 actors=5", NO_ACTOR % fn), (fn + " agent_slot=1 actors=5 critic=0", NO_ACTOR % fn)]
for fn in ("sdc_critic_adam_step", "sdc_get_critic", "sdc_get_critic_optim", "sdc_set_critic_optim", "sdc_set_critic_norm"):
    CASES += [(fn + " actors=0", None), (fn + " critic=0", fn + ": sdc_set_critic first"), (fn + " handle=0 critic=0", fn + ": null handle")]
for fn in ("sdc_get_actor", "sdc_get_critic", "sdc_get_actor_optim", "sdc_get_critic_optim"):
    CASES += [(fn, None), (fn + " out=0", fn + ": null output"), (fn + " handle=0 out=0", fn + ": null handle")]
for fn in ("sdc_set_actor_optim", "sdc_set_critic_optim"):
    CASES += [(fn, None), (fn + " step=0 beta1_pow=1 beta2_pow=1 skipped=0 bad_v=0", None), (fn + " handle=0 m=0", fn + ": null handle")]
    CASES += [("%s %s" % (fn, req), "%s: %s" % (fn, text)) for req, text in STATE_TEXTS]
CASES += [("sdc_set_critic_norm", None), ("sdc_set_critic_norm scale=1e-30 shift=1e30", None),
          ("sdc_set_critic_norm scale=0", "sdc_set_critic_norm: scale must be positive"),
          ("sdc_set_critic_norm scale=-2.5", "sdc_set_critic_norm: scale must be positive"),
          ("sdc_set_critic_norm scale=1e-60", "sdc_set_critic_norm: scale must be positive"),      # (0 as the fp32 the kernels read)
          ("sdc_set_critic_norm scale=nan", "sdc_set_critic_norm: an entry that is not finite"),
          ("sdc_set_critic_norm scale=inf", "sdc_set_critic_norm: an entry that is not finite"),
          ("sdc_set_critic_norm shift=-inf", "sdc_set_critic_norm: an entry that is not finite"),
          ("sdc_set_critic_norm shift=1e60", "sdc_set_critic_norm: an entry that is not finite")]


def ask(exe):
    out = subprocess.run([exe], input="\n".join(c[0] for c in CASES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, (exe, out.returncode, out.stderr[-2000:])
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(CASES)
    return lines


def check(lines):
    wrong = [(req, text, got) for (req, text), got in zip(CASES, lines) if got != ("-" if text is None else text)]
    assert not wrong, wrong[:5]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("optim_refusals"), DRIVER, ["-O1"], "driver")


def test_every_refusal_text(plain):
    check(ask(plain))


def test_every_refusal_text_under_the_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    lines = ask(build(tmp_path, DRIVER, SAN, "driver_san"))
    check(lines)
    assert lines == ask(plain)


def test_the_cases_cover_every_entry_point():
    for fn in ENTRY_POINTS:
        assert any(r.split()[0] == fn and t is None for r, t in CASES) and any(r.split()[0] == fn and t for r, t in CASES), fn
    assert all(t.startswith(r.split()[0] + ": ") for r, t in CASES if t is not None)
