"""The actors on stored rows on the CPU side (sdc_actor_evaluate, sdc_ppo_terms): declared, exported and bound with the ABI still at
313; a null handle is refused before any device work; sdc_actor_eval.hip cross-compiles for gfx950 with no scratch and no spills for
exactly its three kernels; the host pack (csrc/sdc_actor_eval_pack.hpp, built into a small program by the host compiler alone)
un-permutes to its input bit for bit, and a NumPy fp64 forward over the PACKED layout -- in the kernel's data flow -- gives the logits of
a NumPy fp64 forward of the unpacked network to fp64 rounding and the reference's own fp32 logits (tests/golden/actor_eval/actor_eval.npz)
to fp32 rounding; and every text the two calls refuse with (csrc/sdc_refusals.hpp) is held without a GPU in the way
tests/test_onpolicy_abi.py holds its calls': the header compiled by g++ alone into a program that reads one request line per case and
prints the rule's message, or `-` for a call it accepts -- every text below a literal --, plain and built with
-fsanitize=address,undefined (a stand-alone program: nothing is loaded into Python).

A request line:  <entry point> key=value ...   Defaults: a handle of 8 envs with the actors of slots 0 and 2 set, agent 0, n_rows 5,
strides 26 and 3, n_steps 1, clip_param 0.2, every array at a made-up 4096-byte aligned address.  An address is a number (0: NULL),
never followed."""
import os
import subprocess

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import actor_eval_ref as AE
from tests.plan_util import assert_no_scratch_or_spills, entry_point_header, kernel_resources

EVAL_ARGS = ["h", "agent_slot", "obs", "row_stride", "n_rows", "logits", "logits_stride", "stream"]
PPO_ARGS = ["h", "n_steps", "agent", "new_log_probs", "old_log_probs", "entropy", "advantages", "factor", "clip_param", "ratio", "surr",
            "factor_out", "stats", "stream"]
KERNELS = {"sdc_actor_eval_kernel", "sdc_ppo_terms_kernel", "sdc_ppo_stats_kernel"}


def test_entry_points_are_declared_exported_and_bound_at_abi_313():
    entry_point_header("sdc_actor_evaluate", EVAL_ARGS, "sdc_actor_eval.hip")
    entry_point_header("sdc_ppo_terms", PPO_ARGS, "sdc_actor_eval.hip")
    # the Python side's copies of the kernels' plan constants are the header's
    hpp = open(os.path.join(L.CSRC, "sdc_actor_eval.hpp")).read()
    for name, value in (("SDC_ACTOR_EVAL_MAX_BLOCKS", L.ACTOR_EVAL_MAX_BLOCKS), ("SDC_PPO_BLOCK", L.PPO_BLOCK),
                        ("SDC_PPO_MAX_BLOCKS", L.PPO_MAX_BLOCKS), ("SDC_PPO_STATS", L.PPO_STATS)):
        assert "#define %s %d " % (name, value) in hpp.replace("\n", " \n"), name
    from tests import ppo_ref as PR
    assert (PR.BLOCK, PR.MAX_BLOCKS) == (L.PPO_BLOCK, L.PPO_MAX_BLOCKS)


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_actor_evaluate(None, 0, None, 26, 1, None, 3, None) == -2
    assert lib.sdc_last_error() == b"sdc_actor_evaluate: null handle"
    assert lib.sdc_ppo_terms(None, 1, 0, None, None, None, None, None, 0.2, None, None, None, None, None) == -2
    assert lib.sdc_last_error() == b"sdc_ppo_terms: null handle"


def test_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_actor_eval.hip")
    assert_no_scratch_or_spills(per, KERNELS)
    for k, u in per.items():      # (recorded in DESIGN.md section 4.27, not gated)
        print(k, "VGPRs", u.get("VGPRs"), "SGPRs", u.get("TotalSGPRs"), "occupancy", u.get("Occupancy"), "LDS", u.get("LDS Size"))


# ---- the host pack -------------------------------------------------------------------------------------------------------------------
PACK_MAIN = r"""
#include <cstdio>
#include <memory>
#include "%s"
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::unique_ptr<sdc_actor_params> p(new sdc_actor_params);
  std::unique_ptr<SdcActorEvalDev> d(new SdcActorEvalDev);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(p.get(), sizeof(sdc_actor_params), 1, f) != 1) return 2;
  std::fclose(f);
  sdc_actor_eval_pack(p.get(), d.get());
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(d.get(), sizeof(SdcActorEvalDev), 1, f) != 1) return 2;
  std::fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    """csrc/sdc_actor_eval_pack.hpp behind a main(), built by the host compiler alone: params file -> packed file"""
    td = tmp_path_factory.mktemp("actor_eval_pack")
    src = td / "pack_main.cpp"
    src.write_text(PACK_MAIN % os.path.join(L.CSRC, "sdc_actor_eval_pack.hpp"))
    exe = str(td / "pack_main")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, str(src)], check=True)

    def run(params: L.SdcActorParams):
        fin, fout = td / "params.bin", td / "packed.bin"
        fin.write_bytes(bytes(params))
        r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
        assert r.returncode == 0, r
        return AE.parse_packed(fout.read_bytes())

    return run


def _field(p, name):
    return np.ctypeslib.as_array(getattr(p, name)).copy()


@pytest.mark.parametrize("activation,feature_norm", AE.CONFIGS)
def test_pack_unpermutes_to_its_input_and_the_packed_forward_gives_the_fixtures_logits(pack_program, activation, feature_norm):
    from dc_rl_amd.engine import actor_params
    c = AE.case(activation, feature_norm)
    p = actor_params(AE.params(activation, feature_norm))
    d = pack_program(p)
    assert d["flags"] == (1 if feature_norm else 0) | ((activation == "relu") << 1)
    u = AE.unpack(d)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(bits(u["w1"][:, :26]), bits(_field(p, "w1").reshape(64, 26)))
    assert not u["w1"][:, 26:].any() and not u["ln0_g"][26:].any() and not u["ln0_b"][26:].any() and d["b3"][3] == 0      # (the padding is zero)
    assert np.array_equal(bits(u["w2"]), bits(_field(p, "w2").reshape(64, 64)))
    assert np.array_equal(bits(u["w3"]), bits(_field(p, "w3").reshape(3, 64)))
    for mine, theirs in (("b1", "b1"), ("ln1_g", "ln1_gamma"), ("ln1_b", "ln1_beta"), ("b2", "b2"), ("ln2_g", "ln2_gamma"), ("ln2_b", "ln2_beta")):
        assert np.array_equal(bits(u[mine]), bits(_field(p, theirs))), mine
    for mine, theirs in (("ln0_g", "ln0_gamma"), ("ln0_b", "ln0_beta")):
        assert np.array_equal(bits(u[mine][:26]), bits(_field(p, theirs))), mine
    assert np.array_equal(bits(u["b3"][:3]), bits(_field(p, "b3")))
    # every parameter of the fixture is its own value: a swapped pair or a wrong unit would have shown above
    assert len(np.unique(_field(p, "w2"))) > 4000 and len(np.unique(_field(p, "w3"))) == 192
    # the forward over the packed layout, tile by tile (67 rows: four full tiles and three rows on zeros)
    x = np.zeros((80, 26), dtype=np.float32)
    x[:AE.R] = c["obs"]
    got = np.concatenate([AE.packed_forward(d, x[i:i + 16], activation) for i in range(0, 80, 16)])[:AE.R]
    own = AE.forward(c["sd"], c["obs"], activation)
    err_own = np.abs(got - own).max()
    err_ref = np.abs(got - c["logits"].astype(np.float64)).max()
    print("%s: packed fp64 forward against the unpacked fp64 forward %.2e, against the reference's fp32 logits %.2e" % (
        AE.cfg_name(activation, feature_norm), err_own, err_ref))
    assert err_own <= 1e-12, err_own         # fp64 rounding: sums of 64 terms of order one in another order
    assert err_ref <= 2e-4, err_ref          # the reference's logits are fp32 arithmetic: the project's bar for these actors (tests/test_gpu_actor.py)
    # the rows zero-padded as agent_dc's and agent_bat's are among the rows
    assert not c["obs"][1::3, 14:].any() and not c["obs"][2::3, 13:].any() and c["obs"][0::3, 14:].any()


# ---- the refusal texts ---------------------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
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
      f.actor_set[0] = f.actor_set[2] = true;
    }
    if (entry == "sdc_actor_evaluate")
      out(sdc_actor_evaluate_refused(f, (int)I("agent_slot", 0), P<float>("obs"), I("row_stride", 26), I("n_rows", 5), P<float>("logits"),
                                     I("logits_stride", 3)));
    else if (entry == "sdc_ppo_terms")
      out(sdc_ppo_terms_refused(f, (int)I("n_steps", 1), (int)I("agent", 0), P<float>("new_log_probs"), P<float>("old_log_probs"),
                                P<float>("entropy"), P<float>("advantages"), P<float>("factor"), D("clip_param", 0.2), P<float>("ratio"),
                                P<float>("surr"), P<float>("factor_out"), P<double>("stats")));
    else
      return 3;
  }
  return 0;
}
"""

E_NULL = "sdc_actor_evaluate: null array (obs and logits are required)"
E_ALIGN = "sdc_actor_evaluate: obs / logits not dword-aligned"
P_NULL = "sdc_ppo_terms: null array (new_log_probs, old_log_probs, advantages and ratio are required)"
P_ALIGN = "sdc_ppo_terms: new_log_probs / old_log_probs / entropy / advantages / factor / ratio / surr / factor_out not dword-aligned"
ODD = 0x7f0000001002        # an address that is not dword-aligned
FOUR = 0x7f0000001004       # ... dword- but not 8-byte aligned
# (request, the text or None for an accepted call)
CASES = [
    ("sdc_actor_evaluate", None),
    ("sdc_actor_evaluate agent_slot=2 row_stride=78 logits_stride=9 n_rows=2752512", None),
    ("sdc_actor_evaluate n_rows=1 obs=%d logits=%d" % (FOUR, FOUR), None),                       # (dword alignment is all it asks)
    ("sdc_actor_evaluate handle=0", "sdc_actor_evaluate: null handle"),
    ("sdc_actor_evaluate handle=0 agent_slot=7 obs=0", "sdc_actor_evaluate: null handle"),     # (two faults: the handle first)
    ("sdc_actor_evaluate agent_slot=3", "sdc_actor_evaluate: agent_slot = 3 outside [0, 2]"),
    ("sdc_actor_evaluate agent_slot=-1 n_rows=0", "sdc_actor_evaluate: agent_slot = -1 outside [0, 2]"),
    ("sdc_actor_evaluate agent_slot=1", "sdc_actor_evaluate: no actor is set for agent_slot 1 (sdc_set_actor first)"),
    ("sdc_actor_evaluate agent_slot=1 n_rows=0 obs=0", "sdc_actor_evaluate: no actor is set for agent_slot 1 (sdc_set_actor first)"),
    ("sdc_actor_evaluate n_rows=0", "sdc_actor_evaluate: n_rows = 0 must be positive"),
    ("sdc_actor_evaluate n_rows=-4 logits=0", "sdc_actor_evaluate: n_rows = -4 must be positive"),
    ("sdc_actor_evaluate obs=0", E_NULL),
    ("sdc_actor_evaluate logits=0", E_NULL),
    ("sdc_actor_evaluate obs=0 logits=%d row_stride=1" % ODD, E_NULL),
    ("sdc_actor_evaluate obs=%d" % ODD, E_ALIGN),
    ("sdc_actor_evaluate logits=%d row_stride=3" % ODD, E_ALIGN),
    ("sdc_actor_evaluate row_stride=25", "sdc_actor_evaluate: row_stride = 25 below a row's 26 floats"),
    ("sdc_actor_evaluate row_stride=0 logits_stride=0", "sdc_actor_evaluate: row_stride = 0 below a row's 26 floats"),
    ("sdc_actor_evaluate row_stride=-78", "sdc_actor_evaluate: row_stride = -78 below a row's 26 floats"),
    ("sdc_actor_evaluate logits_stride=2", "sdc_actor_evaluate: logits_stride = 2 below a row's 3 floats"),
    ("sdc_actor_evaluate logits_stride=-9", "sdc_actor_evaluate: logits_stride = -9 below a row's 3 floats"),
    ("sdc_ppo_terms", None),
    ("sdc_ppo_terms entropy=0 factor=0 surr=0 factor_out=0 stats=0 n_steps=672 agent=2 clip_param=0", None),      # (what may be NULL)
    ("sdc_ppo_terms clip_param=0.999", None),
    ("sdc_ppo_terms factor=%d factor_out=%d" % (FOUR, FOUR), None),                               # (in place)
    ("sdc_ppo_terms handle=0", "sdc_ppo_terms: null handle"),
    ("sdc_ppo_terms handle=0 n_steps=0 ratio=0", "sdc_ppo_terms: null handle"),
    ("sdc_ppo_terms n_steps=0", "sdc_ppo_terms: n_steps = 0 must be positive"),
    ("sdc_ppo_terms n_steps=-2 agent=9", "sdc_ppo_terms: n_steps = -2 must be positive"),
    ("sdc_ppo_terms agent=3", "sdc_ppo_terms: agent = 3 outside [0, 2]"),
    ("sdc_ppo_terms agent=-1 ratio=0", "sdc_ppo_terms: agent = -1 outside [0, 2]"),
    *[("sdc_ppo_terms %s=0" % a, P_NULL) for a in ("new_log_probs", "old_log_probs", "advantages", "ratio")],
    ("sdc_ppo_terms ratio=0 surr=%d" % ODD, P_NULL),
    *[("sdc_ppo_terms %s=%d" % (a, ODD), P_ALIGN) for a in ("new_log_probs", "old_log_probs", "entropy", "advantages", "factor", "ratio",
                                                           "surr", "factor_out")],
    ("sdc_ppo_terms stats=%d" % FOUR, "sdc_ppo_terms: stats not 8-byte aligned"),
    ("sdc_ppo_terms stats=%d clip_param=2" % ODD, "sdc_ppo_terms: stats not 8-byte aligned"),
    ("sdc_ppo_terms clip_param=1", "sdc_ppo_terms: clip_param = 1.000000 outside [0, 1)"),
    ("sdc_ppo_terms clip_param=-0.1", "sdc_ppo_terms: clip_param = -0.100000 outside [0, 1)"),
    ("sdc_ppo_terms clip_param=nan", "sdc_ppo_terms: clip_param = nan outside [0, 1)"),
    ("sdc_ppo_terms clip_param=inf", "sdc_ppo_terms: clip_param = inf outside [0, 1)"),
]


def build_driver(d, flags, name):
    """the driver built by g++ alone (no HIP on the include path)"""
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + L.CSRC, str(src)] + flags + ["-o", exe], check=True)
    return exe


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
    return build_driver(tmp_path_factory.mktemp("actor_eval_refusals"), ["-O1"], "driver")


def test_every_refusal_text(plain):
    check(ask(plain))


def test_every_refusal_text_under_the_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    san = build_driver(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "driver_san")
    lines = ask(san)
    check(lines)
    assert lines == ask(plain)


def test_the_cases_cover_what_the_header_promises():
    """both calls have an acceptance, and every refusal the header lists for them has its text here"""
    texts = {t for _, t in CASES if t is not None}
    for entry in ("sdc_actor_evaluate", "sdc_ppo_terms"):
        assert any(r.split()[0] == entry and t is None for r, t in CASES) and any(r.split()[0] == entry and t for r, t in CASES)
    assert all(t.startswith(r.split()[0] + ": ") for r, t in CASES if t is not None)
    assert len(texts) == 25
