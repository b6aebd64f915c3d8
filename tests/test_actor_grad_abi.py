"""The actors' gradient on the CPU side (sdc_ppo_dlogp, sdc_actor_backward): declared, exported and bound with the ABI still at 313, the
two constants mirrored; a null handle is refused before any device work; sdc_actor_grad.hip cross-compiles for gfx950 with no scratch and
no spills for exactly its kernels; the transposed pack (csrc/sdc_actor_grad_pack.hpp, built into a small program by the host compiler
alone) un-permutes to its input bit for bit; and every text the two calls refuse with (csrc/sdc_refusals.hpp) is held without a GPU in
the way tests/test_actor_eval_abi.py holds its calls': the header compiled by g++ alone into a program that reads one request line per
case and prints the rule's message, or `-` for a call it accepts -- every text below a literal --, plain and built with
-fsanitize=address,undefined (a stand-alone program: nothing is loaded into Python).

A request line:  <entry point> key=value ...   Defaults: a handle of 8 envs with the actors of slots 0 and 2 set, agent 0, n_rows 5,
strides 26 and 1, n_steps 1, clip_param 0.2, scale 0.125, dent -0.002, every array at a made-up 4096-byte aligned address.  An address is
a number (0: NULL), never followed."""
import os
import re
import subprocess

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import actor_grad_ref as GR
from tests.critic_ref import unit_of_k
from tests.plan_util import assert_no_scratch_or_spills, entry_point_header, kernel_resources

DLOGP_ARGS = ["h", "n_steps", "agent", "new_log_probs", "old_log_probs", "advantages", "factor", "clip_param", "scale", "dlogp", "stream"]
BACKWARD_ARGS = ["h", "agent_slot", "obs", "row_stride", "n_rows", "actions", "action_stride", "dlogp", "dent", "grads", "grad_sq", "stream"]
KERNELS = {"sdc_actor_grad_tanh_kernel", "sdc_actor_grad_relu_kernel", "sdc_actor_grad_reduce_kernel", "sdc_actor_grad_sq_kernel",
           "sdc_ppo_dlogp_kernel"}


def test_entry_points_are_declared_exported_and_bound_at_abi_313():
    hdr = entry_point_header("sdc_ppo_dlogp", DLOGP_ARGS, "sdc_actor_grad.hip")
    entry_point_header("sdc_actor_backward", BACKWARD_ARGS, "sdc_actor_grad.hip")
    for name, value in (("SDC_ACTOR_N_PARAMS", L.ACTOR_N_PARAMS), ("SDC_ACTOR_GRAD_MAX_BLOCKS", L.ACTOR_GRAD_MAX_BLOCKS)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    assert (GR.N_PARAMS, GR.MAX_BLOCKS) == (L.ACTOR_N_PARAMS, L.ACTOR_GRAD_MAX_BLOCKS)
    # the count is the float members of the struct, in the mirror as in the header (the header's static_assert holds the C side)
    floats = [f for f in L.SdcActorParams._fields_ if f[0] not in ("use_feature_normalization", "activation")]
    assert [f[0] for f in floats] == list(GR.FIELDS)
    assert sum(np.prod(GR.SHAPES[k]) for k in GR.FIELDS) == L.ACTOR_N_PARAMS == L.SdcActorParams.use_feature_normalization.offset // 4
    from dc_rl_amd import engine as E
    assert list(E._ACTOR_SHAPES) == list(GR.FIELDS) and all(tuple(E._ACTOR_SHAPES[k]) == GR.SHAPES[k] for k in GR.FIELDS)
    hpp = open(os.path.join(L.CSRC, "sdc_actor_grad.hpp")).read()
    assert "#define SDC_ACTOR_GRAD_SQ_BLOCK %d " % GR.SQ_BLOCK in hpp


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_ppo_dlogp(None, 1, 0, None, None, None, None, 0.2, 1.0, None, None) == -2
    assert lib.sdc_last_error() == b"sdc_ppo_dlogp: null handle"
    assert lib.sdc_actor_backward(None, 0, None, 26, 1, None, 1, None, 0.0, None, None, None) == -2
    assert lib.sdc_last_error() == b"sdc_actor_backward: null handle"


def test_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_actor_grad.hip")
    assert_no_scratch_or_spills(per, KERNELS)
    for k, u in per.items():      # (recorded in DESIGN.md section 4.28, not gated)
        print(k, "VGPRs", u.get("VGPRs"), "AGPRs", u.get("AGPRs"), "SGPRs", u.get("TotalSGPRs"), "occupancy", u.get("Occupancy"), "LDS",
              u.get("LDS Size"))


def test_the_shared_forward_left_the_evaluate_kernels_as_they_were():
    """sdc_actor_eval.hip still holds exactly its three kernels with their resources, and the network they, the critic and the gradient
    kernels run stands ONCE, in csrc/sdc_rowmlp.hpp: the three .hip files include it, and neither they nor the two forward headers hold
    a matrix-instruction layer loop, an epilogue or a LayerNorm's rsq of their own.  The backward stands ONCE as well, in
    csrc/sdc_rowmlp_grad.hpp: its four products (dW2, dY1, dW1, dX) behind the head's forward call; sdc_actor_grad.hip holds its head's
    one (dW3), sdc_critic_grad.hip none"""
    per = kernel_resources("sdc_actor_eval.hip")
    assert_no_scratch_or_spills(per, {"sdc_actor_eval_kernel", "sdc_ppo_terms_kernel", "sdc_ppo_stats_kernel"})
    read = lambda name: open(os.path.join(L.CSRC, name)).read()
    mfma, shared = "__builtin_amdgcn_mfma_f32_16x16x4f32", read("sdc_rowmlp.hpp")
    assert shared.count(mfma) == 2 and len(re.findall(r"\bvoid epilogue\(", shared)) == 1 and shared.count("__builtin_amdgcn_rsqf") == 2
    counts = {"sdc_rowmlp_grad.hpp": 4, "sdc_actor_grad.hip": 1, "sdc_critic_grad.hip": 0}
    for name in ("sdc_critic.hip", "sdc_actor_eval.hip", "sdc_actor_grad.hip", "sdc_critic_grad.hip", "sdc_rowmlp_grad.hpp", "sdc_critic.hpp",
                 "sdc_actor_forward.hpp"):
        src = read(name)
        assert '#include "sdc_rowmlp.hpp"' in src, name
        assert src.count(mfma) == counts.get(name, 0), name
        assert "epilogue" not in src and "__builtin_amdgcn_rsqf" not in src, name
        assert name not in counts or "rsq" not in src, name
    body = read("sdc_rowmlp_grad.hpp")
    assert body.index("HEAD::template forward<KIND>(W, x, lane, out, T)") < body.index(mfma)      # (the four stand behind the forward's call)
    grad = read("sdc_actor_grad.hip")
    assert grad.index("sdc_aev::forward_kind<KIND>(W, x, lane, out.lg, T)") < grad.index(mfma)     # (and dW3 behind the head's forward)
    assert '#include "sdc_rowmlp_grad.hpp"' in grad and grad.index("struct Head {") < grad.index(mfma)


# ---- the transposed pack ------------------------------------------------------------------------------------------------------------
PACK_MAIN = r"""
#include <cstdio>
#include <memory>
#include "%s"
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::unique_ptr<sdc_actor_params> p(new sdc_actor_params);
  std::unique_ptr<SdcActorGradDev> d(new SdcActorGradDev);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(p.get(), sizeof(sdc_actor_params), 1, f) != 1) return 2;
  std::fclose(f);
  sdc_actor_grad_pack(p.get(), d.get());
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(d.get(), sizeof(SdcActorGradDev), 1, f) != 1) return 2;
  std::fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    """csrc/sdc_actor_grad_pack.hpp behind a main(), built by the host compiler alone: params file -> packed file"""
    td = tmp_path_factory.mktemp("actor_grad_pack")
    src = td / "pack_main.cpp"
    src.write_text(PACK_MAIN % os.path.join(L.CSRC, "sdc_actor_grad_pack.hpp"))
    exe = str(td / "pack_main")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, str(src)], check=True)

    def run(params: L.SdcActorParams):
        fin, fout = td / "params.bin", td / "packed.bin"
        fin.write_bytes(bytes(params))
        r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
        assert r.returncode == 0, r
        raw = np.frombuffer(fout.read_bytes(), dtype=np.float32)
        assert raw.size == 16 * 64 * 4 + 16 * 64 * 2
        return raw[:16 * 64 * 4].reshape(16, 64, 4).copy(), raw[16 * 64 * 4:].reshape(16, 64, 2).copy()

    return run


@pytest.mark.parametrize("activation,feature_norm", GR.CONFIGS)
def test_transposed_pack_unpermutes_to_its_input(pack_program, activation, feature_norm):
    from dc_rl_amd.engine import actor_params
    c = GR.case(activation, feature_norm)
    p = actor_params(dict(c["sd"], activation=activation))
    a2t, a1t = pack_program(p)
    w1 = np.ctypeslib.as_array(p.w1).reshape(64, 26)
    w2 = np.ctypeslib.as_array(p.w2).reshape(64, 64)
    u2 = np.full((64, 64), np.nan, np.float32)
    u1 = np.full((64, 32), np.nan, np.float32)
    for s in range(16):
        for l in range(64):
            g, e = l >> 4, l & 15
            unit = unit_of_k(4 * s + g)
            for t in range(4):
                u2[unit, 16 * t + e] = a2t[s, l, t]
            for t in range(2):
                u1[unit, 16 * t + 4 * (e & 3) + (e >> 2)] = a1t[s, l, t]
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(bits(u2), bits(w2)) and np.array_equal(bits(u1[:, :26]), bits(w1)) and not u1[:, 26:].any()
    assert len(np.unique(w2)) > 4000 and len(np.unique(w1)) > 1600      # (every parameter its own value: a swapped pair would have shown)


# ---- the refusal texts -----------------------------------------------------------------------------------------------------------------
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
    if (entry == "sdc_ppo_dlogp")
      out(sdc_ppo_dlogp_refused(f, (int)I("n_steps", 1), (int)I("agent", 0), P<float>("new_log_probs"), P<float>("old_log_probs"),
                                P<float>("advantages"), P<float>("factor"), D("clip_param", 0.2), D("scale", 0.125), P<float>("dlogp")));
    else if (entry == "sdc_actor_backward")
      out(sdc_actor_backward_refused(f, (int)I("agent_slot", 0), P<float>("obs"), I("row_stride", 26), I("n_rows", 5), P<int32_t>("actions"),
                                     I("action_stride", 1), P<float>("dlogp"), D("dent", -0.002), P<float>("grads"), P<double>("grad_sq")));
    else
      return 3;
  }
  return 0;
}
"""

B_NULL = "sdc_actor_backward: null array (obs, actions, dlogp and grads are required)"
B_ALIGN = "sdc_actor_backward: obs / actions / dlogp / grads not dword-aligned"
D_NULL = "sdc_ppo_dlogp: null array (new_log_probs, old_log_probs, advantages and dlogp are required)"
D_ALIGN = "sdc_ppo_dlogp: new_log_probs / old_log_probs / advantages / factor / dlogp not dword-aligned"
ODD = 0x7f0000001002        # an address that is not dword-aligned
FOUR = 0x7f0000001004       # ... dword- but not 8-byte aligned
# (request, the text or None for an accepted call)
CASES = [
    ("sdc_actor_backward", None),
    ("sdc_actor_backward agent_slot=2 row_stride=78 action_stride=3 n_rows=2752512 grad_sq=0 dent=0", None),      # (grad_sq may be NULL)
    ("sdc_actor_backward n_rows=1 obs=%d actions=%d dlogp=%d grads=%d" % (FOUR, FOUR, FOUR, FOUR), None),          # (dword alignment is all they ask)
    ("sdc_actor_backward dent=1e300", None),
    ("sdc_actor_backward handle=0", "sdc_actor_backward: null handle"),
    ("sdc_actor_backward handle=0 agent_slot=7 obs=0", "sdc_actor_backward: null handle"),                         # (two faults: the handle first)
    ("sdc_actor_backward agent_slot=3", "sdc_actor_backward: agent_slot = 3 outside [0, 2]"),
    ("sdc_actor_backward agent_slot=-1 n_rows=0", "sdc_actor_backward: agent_slot = -1 outside [0, 2]"),
    ("sdc_actor_backward agent_slot=1", "sdc_actor_backward: no actor is set for agent_slot 1 (sdc_set_actor first)"),
    ("sdc_actor_backward agent_slot=1 n_rows=0 obs=0", "sdc_actor_backward: no actor is set for agent_slot 1 (sdc_set_actor first)"),
    ("sdc_actor_backward n_rows=0", "sdc_actor_backward: n_rows = 0 must be positive"),
    ("sdc_actor_backward n_rows=-4 grads=0", "sdc_actor_backward: n_rows = -4 must be positive"),
    *[("sdc_actor_backward %s=0" % a, B_NULL) for a in ("obs", "actions", "dlogp", "grads")],
    ("sdc_actor_backward obs=0 grads=%d row_stride=1" % ODD, B_NULL),
    *[("sdc_actor_backward %s=%d" % (a, ODD), B_ALIGN) for a in ("obs", "actions", "dlogp", "grads")],
    ("sdc_actor_backward grad_sq=%d" % FOUR, "sdc_actor_backward: grad_sq not 8-byte aligned"),
    ("sdc_actor_backward grad_sq=%d row_stride=2" % ODD, "sdc_actor_backward: grad_sq not 8-byte aligned"),
    ("sdc_actor_backward row_stride=25", "sdc_actor_backward: row_stride = 25 below a row's 26 floats"),
    ("sdc_actor_backward row_stride=-78 action_stride=0", "sdc_actor_backward: row_stride = -78 below a row's 26 floats"),
    ("sdc_actor_backward action_stride=0", "sdc_actor_backward: action_stride = 0 must be positive"),
    ("sdc_actor_backward action_stride=-3 dent=nan", "sdc_actor_backward: action_stride = -3 must be positive"),
    ("sdc_actor_backward dent=nan", "sdc_actor_backward: dent = nan is not finite"),
    ("sdc_actor_backward dent=-inf", "sdc_actor_backward: dent = -inf is not finite"),
    ("sdc_ppo_dlogp", None),
    ("sdc_ppo_dlogp factor=0 n_steps=672 agent=2 clip_param=0 scale=0", None),                                     # (what may be NULL)
    ("sdc_ppo_dlogp clip_param=0.999 scale=-1e300", None),
    ("sdc_ppo_dlogp handle=0", "sdc_ppo_dlogp: null handle"),
    ("sdc_ppo_dlogp handle=0 n_steps=0 dlogp=0", "sdc_ppo_dlogp: null handle"),
    ("sdc_ppo_dlogp n_steps=0", "sdc_ppo_dlogp: n_steps = 0 must be positive"),
    ("sdc_ppo_dlogp n_steps=-2 agent=9", "sdc_ppo_dlogp: n_steps = -2 must be positive"),
    ("sdc_ppo_dlogp agent=3", "sdc_ppo_dlogp: agent = 3 outside [0, 2]"),
    ("sdc_ppo_dlogp agent=-1 dlogp=0", "sdc_ppo_dlogp: agent = -1 outside [0, 2]"),
    *[("sdc_ppo_dlogp %s=0" % a, D_NULL) for a in ("new_log_probs", "old_log_probs", "advantages", "dlogp")],
    ("sdc_ppo_dlogp dlogp=0 factor=%d" % ODD, D_NULL),
    *[("sdc_ppo_dlogp %s=%d" % (a, ODD), D_ALIGN) for a in ("new_log_probs", "old_log_probs", "advantages", "factor", "dlogp")],
    ("sdc_ppo_dlogp clip_param=1", "sdc_ppo_dlogp: clip_param = 1.000000 outside [0, 1)"),
    ("sdc_ppo_dlogp clip_param=-0.1", "sdc_ppo_dlogp: clip_param = -0.100000 outside [0, 1)"),
    ("sdc_ppo_dlogp clip_param=nan scale=nan", "sdc_ppo_dlogp: clip_param = nan outside [0, 1)"),
    ("sdc_ppo_dlogp scale=nan", "sdc_ppo_dlogp: scale = nan is not finite"),
    ("sdc_ppo_dlogp scale=inf", "sdc_ppo_dlogp: scale = inf is not finite"),
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
    return build_driver(tmp_path_factory.mktemp("actor_grad_refusals"), ["-O1"], "driver")


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
    for entry in ("sdc_actor_backward", "sdc_ppo_dlogp"):
        assert any(r.split()[0] == entry and t is None for r, t in CASES) and any(r.split()[0] == entry and t for r, t in CASES)
    assert all(t.startswith(r.split()[0] + ": ") for r, t in CASES if t is not None)
    assert len(texts) == 27
