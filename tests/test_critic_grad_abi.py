"""The critic's gradient on the CPU side (sdc_critic_evaluate, sdc_value_loss, sdc_critic_backward): declared, exported and bound with the
ABI still at 313, the constants mirrored; a null handle is refused before any device work; sdc_critic_grad.hip cross-compiles for gfx950
with no scratch and no spills for exactly its kernels, next to a shared trunk that gained no matrix instruction; the transposed pack
(csrc/sdc_critic_grad_pack.hpp, built into a small program by the host compiler alone) un-permutes to its input bit for bit and
SdcCriticDev keeps its bytes; and every text the three calls refuse with (csrc/sdc_refusals.hpp) is held without a GPU in the way
tests/test_actor_grad_abi.py holds its calls': the header compiled by g++ alone into a program that reads one request line per case and
prints the rule's message, or `-` for a call it accepts -- every text below a literal --, plain and built with
-fsanitize=address,undefined (a stand-alone program: nothing is loaded into Python).

A request line:  <entry point> key=value ...   Defaults: a handle of 8 envs with a critic set, n_rows 5, n 5, target_scale 2.5,
target_shift -1, clip_param 0.2, huber_delta 10, flags 3, coef 0.2, every array at a made-up 4096-byte aligned address.  An address is a
number (0: NULL), never followed."""
import os
import re
import subprocess

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import critic_grad_ref as GR
from tests.critic_ref import unit_of_k
from tests.plan_util import assert_no_scratch_or_spills, entry_point_header, kernel_resources

EVALUATE_ARGS = ["h", "share_obs", "n_rows", "raw_values", "stream"]
LOSS_ARGS = ["h", "n", "raw_values", "value_preds", "returns", "target_scale", "target_shift", "clip_param", "huber_delta", "flags", "coef",
             "loss", "dvalue", "stats", "stream"]
BACKWARD_ARGS = ["h", "share_obs", "n_rows", "dvalue", "grads", "grad_sq", "stream"]
KERNELS = {"sdc_critic_raw_kernel", "sdc_value_loss_kernel", "sdc_critic_grad_tanh_kernel", "sdc_critic_grad_relu_kernel",
           "sdc_critic_grad_reduce_kernel", "sdc_critic_grad_sq_kernel"}


def test_entry_points_are_declared_exported_and_bound_at_abi_313():
    entry_point_header("sdc_critic_evaluate", EVALUATE_ARGS, "sdc_critic_grad.hip")
    entry_point_header("sdc_value_loss", LOSS_ARGS, "sdc_critic_grad.hip")
    hdr = entry_point_header("sdc_critic_backward", BACKWARD_ARGS, "sdc_critic_grad.hip")
    for name, value in (("SDC_CRITIC_N_PARAMS", L.CRITIC_N_PARAMS), ("SDC_CRITIC_GRAD_MAX_BLOCKS", L.CRITIC_GRAD_MAX_BLOCKS)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    assert (GR.N_PARAMS, GR.MAX_BLOCKS) == (L.CRITIC_N_PARAMS, L.CRITIC_GRAD_MAX_BLOCKS) == (6459, 256)
    assert (GR.HUBER, GR.CLIPPED) == (L.VALUE_LOSS_HUBER, L.VALUE_LOSS_CLIPPED)
    # the count is the float members of the struct up to b3, in the mirror as in the header (the pack header's static_assert holds the C side)
    floats = [f[0] for f in L.SdcCriticParams._fields_ if f[0] not in ("scale", "shift", "flags")]
    assert floats == list(GR.FIELDS)
    assert sum(int(np.prod(GR.SHAPES[k])) for k in GR.FIELDS) == L.CRITIC_N_PARAMS == L.SdcCriticParams.scale.offset // 4
    from dc_rl_amd import engine as E
    assert list(E._CRITIC_SHAPES) == list(GR.FIELDS) and all(tuple(E._CRITIC_SHAPES[k]) == GR.SHAPES[k] for k in GR.FIELDS)
    hpp = open(os.path.join(L.CSRC, "sdc_critic_grad.hpp")).read()
    assert "#define SDC_CRITIC_GRAD_SQ_BLOCK %d " % GR.SQ_BLOCK in hpp
    assert re.search(r"#define SDC_VALUE_LOSS_HUBER 1\b", hpp) and re.search(r"#define SDC_VALUE_LOSS_CLIPPED 2\b", hpp)
    assert "static_assert(SDC_CRITIC_N_PARAMS == offsetof(sdc_critic_params, scale) / 4" in open(os.path.join(L.CSRC, "sdc_critic_grad_pack.hpp")).read()


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_critic_evaluate(None, None, 1, None, None) == -2
    assert lib.sdc_last_error() == b"sdc_critic_evaluate: null handle"
    assert lib.sdc_value_loss(None, 1, None, None, None, 1.0, 0.0, 0.2, 10.0, 3, 1.0, None, None, None, None) == -2
    assert lib.sdc_last_error() == b"sdc_value_loss: null handle"
    assert lib.sdc_critic_backward(None, None, 1, None, None, None, None) == -2
    assert lib.sdc_last_error() == b"sdc_critic_backward: null handle"


def test_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_critic_grad.hip")
    assert_no_scratch_or_spills(per, KERNELS)
    for k, u in per.items():      # (recorded in DESIGN.md section 4.30, not gated)
        print(k, "VGPRs", u.get("VGPRs"), "AGPRs", u.get("AGPRs"), "SGPRs", u.get("TotalSGPRs"), "occupancy", u.get("Occupancy"), "LDS",
              u.get("LDS Size"))


def test_the_critic_backward_stands_next_to_the_actors_over_the_shared_trunk():
    """the trunk stands ONCE, in csrc/sdc_rowmlp.hpp, with the two matrix-instruction loops it had; the backward's four products (dW2,
    dY1, dW1, dX) stand ONCE, in csrc/sdc_rowmlp_grad.hpp, behind the head's forward call; sdc_critic_grad.hip holds its head (the
    trunk's call) and no product, epilogue or LayerNorm rsq of its own; no atomics anywhere in it or in the shared backward"""
    read = lambda name: open(os.path.join(L.CSRC, name)).read()
    mfma, shared = "__builtin_amdgcn_mfma_f32_16x16x4f32", read("sdc_rowmlp.hpp")
    assert shared.count(mfma) == 2 and shared.count("__builtin_amdgcn_rsqf") == 2
    src, body = read("sdc_critic_grad.hip"), read("sdc_rowmlp_grad.hpp")
    assert '#include "sdc_rowmlp.hpp"' in src and '#include "sdc_rowmlp_grad.hpp"' in src and src.count(mfma) == 0 and body.count(mfma) == 4
    for text in (src, body):
        assert "epilogue" not in text and "rsq" not in text and "atomic" not in text.lower()
    assert "sdc_rowmlp::trunk<KIND, SDC_CRITIC_IN>(W, x, lane, out.y2, T)" in src[src.index("struct Head {"):]
    assert body.index("HEAD::template forward<KIND>(W, x, lane, out, T)") < body.index(mfma)
    for name in ("sdc_critic_grad.hpp", "sdc_critic_grad_pack.hpp", "sdc_rowmlp_grad_pack.hpp"):
        assert mfma not in read(name), name
    for name in ("sdc_critic_grad_pack.hpp", "sdc_rowmlp_grad_pack.hpp"):
        assert "hip" not in re.sub(r"//.*", "", read(name)).replace("sustaindc_hip.h", ""), name      # (HIP-free)


# ---- the transposed pack ------------------------------------------------------------------------------------------------------------
PACK_MAIN = r"""
#include <cstdio>
#include <memory>
#include "%s"
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::unique_ptr<sdc_critic_params> p(new sdc_critic_params);
  std::unique_ptr<SdcCriticGradDev> d(new SdcCriticGradDev);
  std::unique_ptr<SdcCriticDev> fwd(new SdcCriticDev);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(p.get(), sizeof(sdc_critic_params), 1, f) != 1) return 2;
  std::fclose(f);
  sdc_critic_grad_pack(p.get(), d.get());
  sdc_critic_pack(p.get(), fwd.get());
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(d.get(), sizeof(SdcCriticGradDev), 1, f) != 1) return 2;
  std::fclose(f);
  f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(fwd.get(), sizeof(SdcCriticDev), 1, f) != 1) return 2;
  std::fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def pack_program(tmp_path_factory):
    """csrc/sdc_critic_grad_pack.hpp behind a main(), built by the host compiler alone: params file -> the two packed files"""
    td = tmp_path_factory.mktemp("critic_grad_pack")
    src = td / "pack_main.cpp"
    src.write_text(PACK_MAIN % os.path.join(L.CSRC, "sdc_critic_grad_pack.hpp"))
    exe = str(td / "pack_main")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, str(src)], check=True)

    def run(params: L.SdcCriticParams):
        fin, fout, ffwd = td / "params.bin", td / "packed.bin", td / "forward.bin"
        fin.write_bytes(bytes(params))
        r = subprocess.run([exe, str(fin), str(fout), str(ffwd)], capture_output=True, text=True)
        assert r.returncode == 0, r
        raw = np.frombuffer(fout.read_bytes(), dtype=np.float32)
        assert raw.size == 16 * 64 * 4 + 16 * 64 * 2
        return raw[:16 * 64 * 4].reshape(16, 64, 4).copy(), raw[16 * 64 * 4:].reshape(16, 64, 2).copy(), ffwd.read_bytes()

    return run


@pytest.mark.parametrize("activation,feature_norm", GR.CONFIGS)
def test_transposed_pack_unpermutes_to_its_input(pack_program, activation, feature_norm):
    from dc_rl_amd.engine import critic_params
    from tests import critic_ref as CR
    c = GR.case(activation, feature_norm)
    p = critic_params(c["sd"], (-3.0, 7.5 ** 2), activation)
    a2t, a1t, fwd = pack_program(p)
    w1 = np.ctypeslib.as_array(p.w1).reshape(64, 29)
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
    assert np.array_equal(bits(u2), bits(w2)) and np.array_equal(bits(u1[:, :29]), bits(w1)) and not u1[:, 29:].any()
    assert len(np.unique(w2)) > 4000 and len(np.unique(w1)) > 1800      # (every parameter its own value: a swapped pair would have shown)
    # SdcCriticDev keeps its bytes: the forward's pack next to it un-permutes as it always did
    assert len(fwd) == CR.PACKED_BYTES
    back = CR.unpack(CR.parse_packed(fwd))
    assert np.array_equal(bits(back["w1"][:, :29]), bits(w1)) and np.array_equal(bits(back["w2"]), bits(w2))


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
      f.critic_set = I("critic", 1) != 0;
    }
    if (entry == "sdc_critic_evaluate")
      out(sdc_critic_evaluate_refused(f, P<float>("share_obs"), I("n_rows", 5), P<float>("raw_values")));
    else if (entry == "sdc_value_loss")
      out(sdc_value_loss_refused(f, I("n", 5), P<float>("raw_values"), P<float>("value_preds"), P<float>("returns"), D("target_scale", 2.5),
                                 D("target_shift", -1.0), D("clip_param", 0.2), D("huber_delta", 10.0), (int)I("flags", 3), D("coef", 0.2),
                                 P<float>("loss"), P<float>("dvalue"), P<double>("stats")));
    else if (entry == "sdc_critic_backward")
      out(sdc_critic_backward_refused(f, P<float>("share_obs"), I("n_rows", 5), P<float>("dvalue"), P<float>("grads"), P<double>("grad_sq")));
    else
      return 3;
  }
  return 0;
}
"""

V_NULL = "sdc_value_loss: null array (raw_values, value_preds, returns and dvalue are required)"
V_ALIGN = "sdc_value_loss: raw_values / value_preds / returns / loss / dvalue not dword-aligned"
B_NULL = "sdc_critic_backward: null array (share_obs, dvalue and grads are required)"
B_ALIGN = "sdc_critic_backward: share_obs / dvalue / grads not dword-aligned"
ODD = 0x7f0000001002        # an address that is not dword-aligned
FOUR = 0x7f0000001004       # ... dword- but not 8-byte aligned
# (request, the text or None for an accepted call)
CASES = [
    ("sdc_critic_evaluate", None),
    ("sdc_critic_evaluate n_rows=2752512 share_obs=%d raw_values=%d" % (FOUR, FOUR), None),                        # (dword alignment is all they ask)
    ("sdc_critic_evaluate handle=0", "sdc_critic_evaluate: null handle"),
    ("sdc_critic_evaluate handle=0 n_rows=0 share_obs=0", "sdc_critic_evaluate: null handle"),                     # (two faults: the handle first)
    ("sdc_critic_evaluate critic=0", "sdc_critic_evaluate: sdc_set_critic first"),
    ("sdc_critic_evaluate critic=0 n_rows=0", "sdc_critic_evaluate: sdc_set_critic first"),
    ("sdc_critic_evaluate n_rows=0", "sdc_critic_evaluate: n_rows = 0 must be positive"),
    ("sdc_critic_evaluate n_rows=-3 raw_values=0", "sdc_critic_evaluate: n_rows = -3 must be positive"),
    ("sdc_critic_evaluate share_obs=0", "sdc_critic_evaluate: null array"),
    ("sdc_critic_evaluate raw_values=0 share_obs=%d" % ODD, "sdc_critic_evaluate: null array"),
    ("sdc_critic_evaluate share_obs=%d" % ODD, "sdc_critic_evaluate: share_obs / raw_values not dword-aligned"),
    ("sdc_critic_evaluate raw_values=%d" % ODD, "sdc_critic_evaluate: share_obs / raw_values not dword-aligned"),
    ("sdc_value_loss", None),
    ("sdc_value_loss critic=0 loss=0 stats=0 flags=0 huber_delta=nan clip_param=0 coef=0 n=2752512", None),        # (what may be NULL; no critic needed;
    ("sdc_value_loss flags=2 huber_delta=-1 target_shift=1e300 coef=-1e300", None),                                #  huber_delta unread without bit 0)
    ("sdc_value_loss flags=1 clip_param=1e9 raw_values=%d loss=%d" % (FOUR, FOUR), None),
    ("sdc_value_loss handle=0", "sdc_value_loss: null handle"),
    ("sdc_value_loss handle=0 n=0 dvalue=0", "sdc_value_loss: null handle"),
    ("sdc_value_loss n=0", "sdc_value_loss: n = 0 must be positive"),
    ("sdc_value_loss n=-7 returns=0", "sdc_value_loss: n = -7 must be positive"),
    *[("sdc_value_loss %s=0" % a, V_NULL) for a in ("raw_values", "value_preds", "returns", "dvalue")],
    ("sdc_value_loss dvalue=0 loss=%d" % ODD, V_NULL),
    *[("sdc_value_loss %s=%d" % (a, ODD), V_ALIGN) for a in ("raw_values", "value_preds", "returns", "loss", "dvalue")],
    ("sdc_value_loss stats=%d" % FOUR, "sdc_value_loss: stats not 8-byte aligned"),
    ("sdc_value_loss stats=%d target_scale=0" % ODD, "sdc_value_loss: stats not 8-byte aligned"),
    ("sdc_value_loss target_scale=0", "sdc_value_loss: target_scale = 0.000000 must be finite and positive"),
    ("sdc_value_loss target_scale=-2.5 clip_param=-1", "sdc_value_loss: target_scale = -2.500000 must be finite and positive"),
    ("sdc_value_loss target_scale=inf", "sdc_value_loss: target_scale = inf must be finite and positive"),
    ("sdc_value_loss target_scale=nan", "sdc_value_loss: target_scale = nan must be finite and positive"),
    ("sdc_value_loss target_shift=nan", "sdc_value_loss: target_shift = nan is not finite"),
    ("sdc_value_loss target_shift=-inf flags=4", "sdc_value_loss: target_shift = -inf is not finite"),
    ("sdc_value_loss clip_param=-0.1", "sdc_value_loss: clip_param = -0.100000 must be finite and not negative"),
    ("sdc_value_loss clip_param=inf", "sdc_value_loss: clip_param = inf must be finite and not negative"),
    ("sdc_value_loss clip_param=nan coef=nan", "sdc_value_loss: clip_param = nan must be finite and not negative"),
    ("sdc_value_loss flags=4", "sdc_value_loss: flags = 4: unknown bits (bit 0: Huber loss, bit 1: clipped value loss)"),
    ("sdc_value_loss flags=-1 huber_delta=0", "sdc_value_loss: flags = -1: unknown bits (bit 0: Huber loss, bit 1: clipped value loss)"),
    ("sdc_value_loss huber_delta=0", "sdc_value_loss: huber_delta = 0.000000 must be finite and positive"),
    ("sdc_value_loss flags=1 huber_delta=-10", "sdc_value_loss: huber_delta = -10.000000 must be finite and positive"),
    ("sdc_value_loss huber_delta=inf", "sdc_value_loss: huber_delta = inf must be finite and positive"),
    ("sdc_value_loss huber_delta=nan coef=inf", "sdc_value_loss: huber_delta = nan must be finite and positive"),
    ("sdc_value_loss coef=nan", "sdc_value_loss: coef = nan is not finite"),
    ("sdc_value_loss coef=-inf", "sdc_value_loss: coef = -inf is not finite"),
    ("sdc_critic_backward", None),
    ("sdc_critic_backward grad_sq=0 n_rows=2752512", None),                                                         # (grad_sq may be NULL)
    ("sdc_critic_backward n_rows=1 share_obs=%d dvalue=%d grads=%d" % (FOUR, FOUR, FOUR), None),
    ("sdc_critic_backward handle=0", "sdc_critic_backward: null handle"),
    ("sdc_critic_backward handle=0 n_rows=0 grads=0", "sdc_critic_backward: null handle"),
    ("sdc_critic_backward critic=0", "sdc_critic_backward: sdc_set_critic first"),
    ("sdc_critic_backward critic=0 dvalue=0", "sdc_critic_backward: sdc_set_critic first"),
    ("sdc_critic_backward n_rows=0", "sdc_critic_backward: n_rows = 0 must be positive"),
    ("sdc_critic_backward n_rows=-4 grads=0", "sdc_critic_backward: n_rows = -4 must be positive"),
    *[("sdc_critic_backward %s=0" % a, B_NULL) for a in ("share_obs", "dvalue", "grads")],
    ("sdc_critic_backward share_obs=0 grads=%d" % ODD, B_NULL),
    *[("sdc_critic_backward %s=%d" % (a, ODD), B_ALIGN) for a in ("share_obs", "dvalue", "grads")],
    ("sdc_critic_backward grad_sq=%d" % FOUR, "sdc_critic_backward: grad_sq not 8-byte aligned"),
    ("sdc_critic_backward grad_sq=%d" % ODD, "sdc_critic_backward: grad_sq not 8-byte aligned"),
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
    return build_driver(tmp_path_factory.mktemp("critic_grad_refusals"), ["-O1"], "driver")


def test_every_refusal_text(plain):
    check(ask(plain))


def test_every_refusal_text_under_the_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    san = build_driver(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "driver_san")
    lines = ask(san)
    check(lines)
    assert lines == ask(plain)


def test_the_cases_cover_what_the_header_promises():
    """every call has an acceptance, and every refusal the header lists for it has its text here"""
    texts = {t for _, t in CASES if t is not None}
    for entry in ("sdc_critic_evaluate", "sdc_value_loss", "sdc_critic_backward"):
        assert any(r.split()[0] == entry and t is None for r, t in CASES) and any(r.split()[0] == entry and t for r, t in CASES)
    assert all(t.startswith(r.split()[0] + ": ") for r, t in CASES if t is not None)
    assert len(texts) == 36
