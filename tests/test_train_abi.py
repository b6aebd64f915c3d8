"""TRAIN ON THE DEVICE on the CPU side (include/sustaindc_hip.h): the six entry points declared, exported and bound with the ABI still
at 313 and their two structs mirrored; a null handle refused before any device work; sdc_minibatch.hip cross-compiles for gfx950 with
no scratch and no spills for exactly its kernels; and two stand-alone programs built by the host compiler alone with
-ffp-contract=off, plain and with -fsanitize=address,undefined (nothing is loaded into Python):
  (a) csrc/sdc_minibatch.hpp's permutation and ValueNorm update equal the NumPy restatement tests/train_ref.py bit for bit;
  (b) every text the new calls refuse with (csrc/sdc_refusals.hpp): one request line per case in, the rule's message or `-` out.

A request line of (b):  <entry point> key=value ...   Defaults: a handle with a critic set and a ValueNorm installed, every array at a
made-up 4096-byte aligned address (a number, 0: NULL, never followed), three good gather segments of 1, 26 and 29 dwords (`seg=<g>`
with `src`, `dst`, `n_dwords`, `src_stride`, `dst_stride` changes segment g), a good sdc_value_norm, n = 800, beta 0.99999."""
import os
import struct
import subprocess

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import train_ref as TR
from tests.plan_util import assert_c_layout, assert_no_scratch_or_spills, entry_point_header, kernel_resources

LOSS_ARGS = ["h", "n", "raw_values", "value_preds", "returns", "clip_param", "huber_delta", "flags", "coef", "loss", "dvalue", "stats", "stream"]
ENTRY_POINTS = {
    "sdc_permutation": ["h", "n", "seed", "stream_id", "perm", "stream"],
    "sdc_gather_rows": ["h", "idx", "n_rows", "n_src_rows", "segs", "n_segs", "bad", "stream"],
    "sdc_set_value_norm": ["h", "st"],
    "sdc_get_value_norm": ["h", "out"],
    "sdc_value_norm_update": ["h", "returns", "n", "beta", "stream"],
    "sdc_value_loss_normed": LOSS_ARGS,
}
KERNELS = {"sdc_permutation_kernel", "sdc_gather_rows_kernel", "sdc_value_norm_sums_kernel", "sdc_value_norm_update_kernel",
           "sdc_value_loss_normed_kernel"}
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
CXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I" + L.CSRC]


def test_entry_points_are_declared_exported_and_bound_at_abi_313(tmp_path):
    for fn, args in ENTRY_POINTS.items():
        hdr = entry_point_header(fn, args, "sdc_minibatch.hip")
    assert_c_layout(tmp_path, "sdc_value_norm", L.SdcValueNorm, ["running_mean", "running_mean_sq", "debiasing_term"])
    assert_c_layout(tmp_path, "sdc_gather_segment", L.SdcGatherSegment, ["src", "dst", "src_stride", "dst_stride", "n_dwords"])
    assert "#define SDC_GATHER_MAX_SEGMENTS %d\n" % L.GATHER_MAX_SEGMENTS in hdr
    hpp = open(os.path.join(L.CSRC, "sdc_minibatch.hpp")).read()
    assert "#define SDC_PERM_ROUNDS %d\n" % TR.ROUNDS in hpp
    assert "#define SDC_VN_BLOCK %d " % TR.BLOCK in hpp and "#define SDC_VN_MAX_BLOCKS %d " % TR.MAX_BLOCKS in hpp
    assert (TR.BLOCK, TR.MAX_BLOCKS) == (L.PPO_BLOCK, L.PPO_MAX_BLOCKS)
    assert "#define SDC_PERM_MAX_N %dll" % L.PERM_MAX_N in hpp
    assert "NOT A UNIFORM DRAW FROM ALL n! PERMUTATIONS" in hpp
    for name in ("sdc_minibatch.hpp", "sdc_philox.hpp"):      # (HIP-free but for the markers)
        src = open(os.path.join(L.CSRC, name)).read()
        assert "hip_runtime" not in src and "hipStream" not in src and "sdc_handle" not in src.split("#pragma once")[1], name


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    calls = {
        "sdc_permutation": lambda: lib.sdc_permutation(None, 8, 1, 0, None, None),
        "sdc_gather_rows": lambda: lib.sdc_gather_rows(None, None, 1, 1, None, 1, None, None),
        "sdc_set_value_norm": lambda: lib.sdc_set_value_norm(None, None),
        "sdc_get_value_norm": lambda: lib.sdc_get_value_norm(None, None),
        "sdc_value_norm_update": lambda: lib.sdc_value_norm_update(None, None, 1, 0.5, None),
        "sdc_value_loss_normed": lambda: lib.sdc_value_loss_normed(None, 1, None, None, None, 0.2, 10.0, 3, 1.0, None, None, None, None),
    }
    assert set(calls) == set(ENTRY_POINTS)
    for fn, call in calls.items():
        assert call() == -2 and lib.sdc_last_error() == (fn + ": null handle").encode(), fn


def test_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_minibatch.hip")
    assert_no_scratch_or_spills(per, KERNELS)
    for k, u in per.items():      # (recorded in DESIGN.md section 4.32, not gated)
        print(k, "VGPRs", u.get("VGPRs"), "SGPRs", u.get("TotalSGPRs"), "occupancy", u.get("Occupancy"), "LDS", u.get("LDS Size"))
    src = open(os.path.join(L.CSRC, "sdc_minibatch.hip")).read()
    assert "atomic" not in src.lower() and "#pragma clang fp contract(off)" in src
    # the value loss' pass stands once, under both of its kernels
    shared = open(os.path.join(L.CSRC, "sdc_value_loss_dev.hpp")).read()
    assert shared.count("void value_loss_pass(") == 1
    for name in ("sdc_minibatch.hip", "sdc_critic_grad.hip"):
        text = open(os.path.join(L.CSRC, name)).read()
        assert '#include "sdc_value_loss_dev.hpp"' in text and "void value_loss_pass(" not in text, name


def build(td, text, flags, name):
    src = td / (name + ".cpp")
    src.write_text(text)
    exe = str(td / name)
    subprocess.run(CXX + [str(src)] + flags + ["-o", exe], check=True)
    return exe


# ---- (a) the header's arithmetic against the restatement --------------------------------------------------------------------------------
ARITH_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sdc_minibatch.hpp"
// perm <n> <seed> <stream_id> <out>: the permutation as int32 [n]
// vn <in> <out>: in: int64 n_updates, double beta, float state[3]; per update int64 n, float x[n].  out, per update: SdcValueNormDev
int main(int argc, char** argv) {
  if (argc == 6 && !std::strcmp(argv[1], "perm")) {
    const long long n = std::strtoll(argv[2], nullptr, 0);
    std::vector<int32_t> perm((size_t)n);
    sdc_permutation_host(n, std::strtoull(argv[3], nullptr, 0), std::strtoull(argv[4], nullptr, 0), perm.data());
    FILE* o = std::fopen(argv[5], "wb");
    if (!o || std::fwrite(perm.data(), 4, (size_t)n, o) != (size_t)n) return 2;
    std::fclose(o);
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "vn")) {
    FILE* f = std::fopen(argv[2], "rb");
    FILE* o = std::fopen(argv[3], "wb");
    long long updates;
    double beta;
    SdcValueNormDev s{};
    if (!f || !o || std::fread(&updates, 8, 1, f) != 1 || std::fread(&beta, 8, 1, f) != 1 || std::fread(&s, 4, 3, f) != 3) return 2;
    sdc_value_norm_derive(s);
    for (long long u = 0; u < updates; u++) {
      long long n;
      if (std::fread(&n, 8, 1, f) != 1) return 2;
      std::vector<float> x((size_t)n);
      if (std::fread(x.data(), 4, (size_t)n, f) != (size_t)n) return 2;
      sdc_value_norm_update_host(s, x.data(), n, beta);
      std::fwrite(&s, sizeof(s), 1, o);
    }
    std::fclose(f);
    std::fclose(o);
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module")
def arith_programs(tmp_path_factory):
    td = tmp_path_factory.mktemp("train_arith")
    return td, [build(td, ARITH_MAIN, ["-O2"], "arith"), build(td, ARITH_MAIN, SAN, "arith_san")]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 800, 1025, 4097])
def test_header_permutation_equals_the_restatement_bit_for_bit(arith_programs, n):
    td, exes = arith_programs
    for seed, stream in ((20260101, (2 << 32) | 3), ((0xDEADBEEF << 32) | 5, 0)):
        want = TR.permutation(n, seed, stream)[0]
        for exe in exes:
            out = td / "perm.bin"
            r = subprocess.run([exe, "perm", str(n), str(seed), str(stream), str(out)], capture_output=True, text=True)
            assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
            assert np.array_equal(np.fromfile(out, dtype=np.int32), want), (exe, n, seed, stream)


def test_header_permutation_at_the_flagship_size(arith_programs):
    td, exes = arith_programs
    n = 672 * 4096
    want = TR.permutation(n, 11, (3 << 32) | 4)[0]
    out = td / "perm_big.bin"
    r = subprocess.run([exes[0], "perm", str(n), "11", str((3 << 32) | 4), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert np.array_equal(np.fromfile(out, dtype=np.int32), want)


@pytest.mark.parametrize("n", [1, 63, 800, 262144 + 77])
def test_header_value_norm_update_equals_the_restatement_bit_for_bit(arith_programs, n):
    td, exes = arith_programs
    rng = np.random.default_rng(n)
    beta, start = 0.99999, (np.float32(-0.25), np.float32(1.5), np.float32(0.125))
    xs = [(rng.normal(-3.0, 2.0, n) * (1 + 0.3 * u)).astype(np.float32) for u in range(5)]
    want, st = [], start
    for x in xs:
        st, (scale, shift) = TR.value_norm_update(st, x, beta)
        want.append(np.array([*st, scale, shift], dtype=np.float32))
    fin, fout = td / "vn_in.bin", td / "vn_out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<qd3f", len(xs), beta, *map(float, start)))
        for x in xs:
            f.write(struct.pack("<q", x.size) + x.tobytes())
    for exe in exes:
        r = subprocess.run([exe, "vn", str(fin), str(fout)], capture_output=True, text=True)
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        got = np.fromfile(fout, dtype=np.float32).reshape(len(xs), 5)
        assert np.array_equal(got.view(np.uint32), np.array(want).view(np.uint32)), (exe, n, got, want)


# ---- (b) the refusal texts -------------------------------------------------------------------------------------------------------------
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
    }
    const bool installed = I("installed", 1) != 0;
    if (entry == "sdc_permutation") {
      out(sdc_permutation_refused(f, I("n", 800), P<int32_t>("perm")));
    } else if (entry == "sdc_gather_rows") {
      std::vector<sdc_gather_segment> segs((size_t)(I("n_segs", 3) > 0 && I("n_segs", 3) <= 64 ? I("n_segs", 3) : 3));
      const int widths[3] = {1, 26, 29};
      for (size_t g = 0; g < segs.size(); g++)
        segs[g] = sdc_gather_segment{P<void>("-"), P<void>("-", GOOD + 0x100000), 78, 78, widths[g % 3]};
      if (R.count("seg")) {
        sdc_gather_segment& g = segs[(size_t)I("seg", 0)];
        g = sdc_gather_segment{P<void>("src"), P<void>("dst", GOOD + 0x100000), I("src_stride", 78), I("dst_stride", 78), (int)I("n_dwords", 26)};
      }
      out(sdc_gather_rows_refused(f, P<int32_t>("idx"), I("n_rows", 400), I("n_src_rows", 800), I("segs", 1) ? segs.data() : nullptr,
                                  (int)I("n_segs", 3), P<int32_t>("bad")));
    } else if (entry == "sdc_set_value_norm") {
      sdc_value_norm st{(float)D("running_mean", -0.5), (float)D("running_mean_sq", 2.0), (float)D("debiasing_term", 0.25)};
      out(sdc_set_value_norm_refused(f, I("st", 1) ? &st : nullptr));
    } else if (entry == "sdc_get_value_norm") {
      out(sdc_get_value_norm_refused(f, installed, P<sdc_value_norm>("out")));
    } else if (entry == "sdc_value_norm_update") {
      out(sdc_value_norm_update_refused(f, installed, P<float>("returns"), I("n", 800), D("beta", 0.99999)));
    } else if (entry == "sdc_value_loss_normed") {
      out(sdc_value_loss_normed_refused(f, installed, I("n", 800), P<float>("raw_values"), P<float>("value_preds"), P<float>("returns"),
                                        D("clip_param", 0.2), D("huber_delta", 10.0), (int)I("flags", 3), D("coef", 1.0 / 800), P<float>("loss"),
                                        P<float>("dvalue"), P<double>("stats")));
    } else {
      return 3;
    }
  }
  return 0;
}
"""

ODD, FOUR = 0x7f0000001002, 0x7f0000001004
NOT_INSTALLED = "%s: no ValueNorm is installed (sdc_set_value_norm first)"
CASES = [
    ("sdc_permutation", None), ("sdc_permutation n=1", None), ("sdc_permutation n=2147483647 perm=%d" % FOUR, None),
    ("sdc_permutation critic=0 installed=0", None),
    ("sdc_permutation handle=0 n=0", "sdc_permutation: null handle"),
    ("sdc_permutation n=0", "sdc_permutation: n = 0 outside [1, 2147483647]"),
    ("sdc_permutation n=-5 perm=0", "sdc_permutation: n = -5 outside [1, 2147483647]"),
    ("sdc_permutation n=2147483648", "sdc_permutation: n = 2147483648 outside [1, 2147483647]"),
    ("sdc_permutation perm=0", "sdc_permutation: null perm"),
    ("sdc_permutation perm=%d" % ODD, "sdc_permutation: perm not dword-aligned"),
    ("sdc_gather_rows", None), ("sdc_gather_rows bad=0 n_segs=16 n_rows=1 n_src_rows=1", None), ("sdc_gather_rows critic=0 installed=0", None),
    ("sdc_gather_rows seg=2 n_dwords=1 src_stride=1 dst_stride=1 src=%d dst=%d" % (FOUR, FOUR + 4096), None),
    ("sdc_gather_rows handle=0 idx=0", "sdc_gather_rows: null handle"),
    ("sdc_gather_rows n_rows=0", "sdc_gather_rows: n_rows = 0 must be positive"),
    ("sdc_gather_rows n_src_rows=0", "sdc_gather_rows: n_src_rows = 0 outside [1, 2147483647]"),
    ("sdc_gather_rows n_src_rows=2147483648", "sdc_gather_rows: n_src_rows = 2147483648 outside [1, 2147483647]"),
    ("sdc_gather_rows idx=0", "sdc_gather_rows: null idx or segs"), ("sdc_gather_rows segs=0", "sdc_gather_rows: null idx or segs"),
    ("sdc_gather_rows idx=%d" % ODD, "sdc_gather_rows: idx / bad not dword-aligned"),
    ("sdc_gather_rows bad=%d" % ODD, "sdc_gather_rows: idx / bad not dword-aligned"),
    ("sdc_gather_rows n_segs=0", "sdc_gather_rows: n_segs = 0 outside [1, 16]"),
    ("sdc_gather_rows n_segs=17", "sdc_gather_rows: n_segs = 17 outside [1, 16]"),
    ("sdc_gather_rows seg=1 src=0", "sdc_gather_rows: segment 1: a null src or dst"),
    ("sdc_gather_rows seg=0 dst=0", "sdc_gather_rows: segment 0: a null src or dst"),
    ("sdc_gather_rows seg=2 src=%d" % ODD, "sdc_gather_rows: segment 2: src / dst not dword-aligned"),
    ("sdc_gather_rows seg=2 dst=%d" % ODD, "sdc_gather_rows: segment 2: src / dst not dword-aligned"),
    ("sdc_gather_rows seg=1 n_dwords=0", "sdc_gather_rows: segment 1: n_dwords must be positive"),
    ("sdc_gather_rows seg=1 n_dwords=27 src_stride=26", "sdc_gather_rows: segment 1: a stride below n_dwords"),
    ("sdc_gather_rows seg=1 n_dwords=27 dst_stride=26", "sdc_gather_rows: segment 1: a stride below n_dwords"),
    ("sdc_set_value_norm", None), ("sdc_set_value_norm st=0", None), ("sdc_set_value_norm installed=0", None),
    ("sdc_set_value_norm running_mean=0 running_mean_sq=0 debiasing_term=0", None),
    ("sdc_set_value_norm handle=0 st=0", "sdc_set_value_norm: null handle"),
    ("sdc_set_value_norm critic=0", "sdc_set_value_norm: sdc_set_critic first"),
    ("sdc_set_value_norm running_mean=nan", "sdc_set_value_norm: an entry that is not finite"),
    ("sdc_set_value_norm running_mean_sq=inf", "sdc_set_value_norm: an entry that is not finite"),
    ("sdc_set_value_norm debiasing_term=1e60", "sdc_set_value_norm: an entry that is not finite"),
    ("sdc_set_value_norm running_mean_sq=-1", "sdc_set_value_norm: running_mean_sq and debiasing_term must not be negative"),
    ("sdc_set_value_norm debiasing_term=-1e-9", "sdc_set_value_norm: running_mean_sq and debiasing_term must not be negative"),
    ("sdc_set_value_norm running_mean=1e36 debiasing_term=1e-5", "sdc_set_value_norm: the debiased mean or variance is not finite"),
    ("sdc_get_value_norm", None),
    ("sdc_get_value_norm handle=0 out=0", "sdc_get_value_norm: null handle"),
    ("sdc_get_value_norm critic=0", "sdc_get_value_norm: sdc_set_critic first"),
    ("sdc_get_value_norm installed=0 out=0", NOT_INSTALLED % "sdc_get_value_norm"),
    ("sdc_get_value_norm out=0", "sdc_get_value_norm: null output"),
    ("sdc_value_norm_update", None), ("sdc_value_norm_update n=1 beta=0 returns=%d" % FOUR, None),
    ("sdc_value_norm_update handle=0 n=0", "sdc_value_norm_update: null handle"),
    ("sdc_value_norm_update critic=0 installed=0", "sdc_value_norm_update: sdc_set_critic first"),
    ("sdc_value_norm_update installed=0 n=0", NOT_INSTALLED % "sdc_value_norm_update"),
    ("sdc_value_norm_update n=0", "sdc_value_norm_update: n = 0 must be positive"),
    ("sdc_value_norm_update returns=0", "sdc_value_norm_update: null returns"),
    ("sdc_value_norm_update returns=%d" % ODD, "sdc_value_norm_update: returns not dword-aligned"),
    ("sdc_value_norm_update beta=1", "sdc_value_norm_update: beta = 1.000000 outside [0, 1)"),
    ("sdc_value_norm_update beta=-0.5", "sdc_value_norm_update: beta = -0.500000 outside [0, 1)"),
    ("sdc_value_norm_update beta=nan", "sdc_value_norm_update: beta = nan outside [0, 1)"),
    ("sdc_value_loss_normed", None), ("sdc_value_loss_normed loss=0 stats=0 flags=0", None),
    ("sdc_value_loss_normed handle=0", "sdc_value_loss_normed: null handle"),
    ("sdc_value_loss_normed installed=0", NOT_INSTALLED % "sdc_value_loss_normed"),
    ("sdc_value_loss_normed n=0 installed=0", "sdc_value_loss_normed: n = 0 must be positive"),
    ("sdc_value_loss_normed dvalue=0", "sdc_value_loss_normed: null array (raw_values, value_preds, returns and dvalue are required)"),
    ("sdc_value_loss_normed returns=%d" % ODD, "sdc_value_loss_normed: raw_values / value_preds / returns / loss / dvalue not dword-aligned"),
    ("sdc_value_loss_normed stats=%d" % FOUR, "sdc_value_loss_normed: stats not 8-byte aligned"),
    ("sdc_value_loss_normed clip_param=-0.1", "sdc_value_loss_normed: clip_param = -0.100000 must be finite and not negative"),
    ("sdc_value_loss_normed flags=4", "sdc_value_loss_normed: flags = 4: unknown bits (bit 0: Huber loss, bit 1: clipped value loss)"),
    ("sdc_value_loss_normed huber_delta=0", "sdc_value_loss_normed: huber_delta = 0.000000 must be finite and positive"),
    ("sdc_value_loss_normed coef=inf", "sdc_value_loss_normed: coef = inf is not finite"),
]


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
    return build(tmp_path_factory.mktemp("train_refusals"), DRIVER, ["-O1"], "driver")


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


def test_the_binding_side_rules_without_a_gpu():
    """dc_rl_amd/_args.py: which dwords a mini-batch gathers, how a batch is cut, the permutation's stream ids"""
    from dc_rl_amd import _args as A
    full = A.minibatch_segments()
    assert [s[0] for s in full] == list(A.MINIBATCH_FIELDS) and len(full) + 1 <= L.GATHER_MAX_SEGMENTS
    assert sum(s[2] for s in full) == 78 + 3 + 9 + 3 + 3 + 1 + 29 + 1 + 1 + 1 + 3 + 1
    one = A.minibatch_segments(agent=1, critic=False)
    assert one == [("obs", 26, 26, 78), ("actions", 1, 1, 3), ("logits", 3, 3, 9), ("action_log_probs", 1, 1, 3), ("entropy", 1, 1, 3),
                   ("advantages", 0, 1, 1)]
    assert 3 * sum(s[2] for s in one) - 2 == sum(s[2] for s in A.minibatch_segments(critic=False))      # (a third of the per-agent dwords)
    assert [s[0] for s in A.minibatch_segments(actors=False)] == ["share_obs", "values", "value_preds", "returns"]
    assert A.minibatch_rows("t", 20, 40, 2) == 400 and A.minibatch_rows("t", 20, 40, 5) == 160 and A.minibatch_rows("t", 20, 40, 1) == 800
    for bad in (3, 0, -1, 2.0, True):
        with pytest.raises(ValueError, match="num_mini_batch"):
            A.minibatch_rows("t", 20, 40, bad)
    assert A.perm_stream_id(2, 4) == (2 << 32) | 4 and A.perm_stream_id(3, 0) == 3 << 32
    st = A.value_norm_struct("t", dict(running_mean=np.float32(-0.5), running_mean_sq=2.0, debiasing_term=0.25))
    assert (st.running_mean, st.running_mean_sq, st.debiasing_term) == (-0.5, 2.0, 0.25)
    st = A.value_norm_struct("t", (0.5, 4.0))
    assert (st.running_mean, st.running_mean_sq, st.debiasing_term) == (0.5, 4.25, 1.0)
    assert A.value_norm_struct("t", None) is None
    with pytest.raises(KeyError, match="running_mean"):
        A.value_norm_struct("t", dict(mean=0.0))
    with pytest.raises(ValueError, match="pair"):
        A.value_norm_struct("t", (1.0, 2.0, 3.0))
