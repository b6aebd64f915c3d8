"""The on-policy batch on the CPU side (sdc_gae, sdc_action_log_probs): declared, exported and bound with the ABI still at 313; a null
handle is refused before any device work; sdc_onpolicy.hip cross-compiles for gfx950 with no scratch and no spills for exactly its
three kernels; and every text the two calls refuse with (csrc/sdc_refusals.hpp) is held without a GPU, in the way
tests/test_host_refusals.py holds the others: the header compiled by g++ alone into a program that reads one request line per case and
prints the rule's message, or `-` for a call it accepts -- every text below a literal, none built by the code under test; the same
cases run through the same program built with -fsanitize=address,undefined (a stand-alone program: nothing is loaded into Python).

A request line:  <entry point> key=value ...   Defaults: a handle of 8 envs without a critic, n_steps 1, every array at a made-up
4096-byte aligned address, gamma 0.99, gae_lambda 0.95, use_gae 1, reward_agent 0.  An address is a number (0: NULL), never followed."""
import subprocess

import pytest

from dc_rl_amd import _lib as L
from tests.plan_util import assert_no_scratch_or_spills, entry_point_header, kernel_resources

GAE_ARGS = ["h", "n_steps", "rew", "reward_agent", "done", "first_done", "values", "gamma", "gae_lambda", "use_gae", "returns",
            "advantages", "masks", "value_preds", "moments", "stream"]
LOGP_ARGS = ["h", "n_steps", "actions", "logits", "log_probs", "entropy", "stream"]
KERNELS = {"sdc_gae_kernel", "sdc_adv_moments_kernel", "sdc_action_logp_kernel"}


def test_entry_points_are_declared_exported_and_bound_at_abi_313():
    entry_point_header("sdc_gae", GAE_ARGS, "sdc_onpolicy.hip")
    entry_point_header("sdc_action_log_probs", LOGP_ARGS, "sdc_onpolicy.hip")


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_gae(None, 1, None, 0, None, None, None, 0.99, 0.95, 1, None, None, None, None, None, None) == -2
    assert lib.sdc_last_error() == b"sdc_gae: null handle"
    assert lib.sdc_action_log_probs(None, 1, None, None, None, None, None) == -2
    assert lib.sdc_last_error() == b"sdc_action_log_probs: null handle"


def test_kernels_compile_for_gfx950_without_scratch_or_spills():
    per = kernel_resources("sdc_onpolicy.hip")
    assert_no_scratch_or_spills(per, KERNELS)
    for k, u in per.items():      # (recorded in DESIGN.md section 4.26, not gated)
        print(k, "VGPRs", u.get("VGPRs"), "SGPRs", u.get("TotalSGPRs"), "occupancy", u.get("Occupancy"), "LDS", u.get("LDS Size"))


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
      f.critic_set = I("critic", 0) != 0;
    }
    const int n_steps = (int)I("n_steps", 1);
    if (entry == "sdc_gae")
      out(sdc_gae_refused(f, n_steps, P<float>("rew"), (int)I("reward_agent", 0), P<uint8_t>("done"), P<float>("values"), D("gamma", 0.99),
                          D("gae_lambda", 0.95), (int)I("use_gae", 1), P<float>("returns"), P<float>("advantages"), P<float>("masks"),
                          P<float>("value_preds", 0), P<double>("moments")));
    else if (entry == "sdc_action_log_probs")
      out(sdc_action_log_probs_refused(f, n_steps, P<int32_t>("actions"), P<float>("logits"), P<float>("log_probs"), P<float>("entropy")));
    else
      return 3;
  }
  return 0;
}
"""

G_NULL = "sdc_gae: null array (rew, done, values, returns, advantages and masks are required)"
G_ALIGN = "sdc_gae: rew / values / returns / advantages / masks / value_preds not dword-aligned"
A_NULL = "sdc_action_log_probs: null array (actions, logits and log_probs are required)"
A_ALIGN = "sdc_action_log_probs: actions / logits / log_probs / entropy not dword-aligned"
ODD = 0x7f0000001002        # an address that is not dword-aligned
EIGHT = 0x7f0000001008      # ... dword- but not 16-byte aligned
# (request, the text or None for an accepted call)
CASES = [
    ("sdc_gae", None),
    ("sdc_gae critic=1 value_preds=%d" % 0x7f0000002000, None),
    ("sdc_gae moments=0 n_steps=672 gamma=1 gae_lambda=1 use_gae=0 reward_agent=2", None),      # (moments may be NULL)
    ("sdc_gae gamma=0 gae_lambda=0", None),
    ("sdc_gae done=%d" % 0x7f0000001001, None),                                                    # (done is bytes: any address)
    ("sdc_gae handle=0", "sdc_gae: null handle"),
    ("sdc_gae handle=0 n_steps=0 rew=0", "sdc_gae: null handle"),                               # (two faults: the handle first)
    ("sdc_gae n_steps=0", "sdc_gae: n_steps = 0 must be positive"),
    ("sdc_gae n_steps=-3 rew=0", "sdc_gae: n_steps = -3 must be positive"),
    *[("sdc_gae %s=0" % a, G_NULL) for a in ("rew", "done", "values", "returns", "advantages", "masks")],
    ("sdc_gae rew=0 reward_agent=5", G_NULL),
    *[("sdc_gae %s=%d" % (a, ODD), G_ALIGN) for a in ("rew", "values", "returns", "advantages", "masks")],
    ("sdc_gae critic=1 value_preds=%d" % ODD, G_ALIGN),
    ("sdc_gae value_preds=%d" % ODD, G_ALIGN),                                                   # (before the missing critic)
    ("sdc_gae moments=%d" % EIGHT, "sdc_gae: moments not 16-byte aligned"),
    ("sdc_gae moments=%d reward_agent=3" % EIGHT, "sdc_gae: moments not 16-byte aligned"),
    ("sdc_gae reward_agent=3", "sdc_gae: reward_agent = 3 outside [0, 2]"),
    ("sdc_gae reward_agent=-1 use_gae=2", "sdc_gae: reward_agent = -1 outside [0, 2]"),
    ("sdc_gae use_gae=2", "sdc_gae: use_gae = 2 outside {0, 1}"),
    ("sdc_gae use_gae=-1 gamma=2", "sdc_gae: use_gae = -1 outside {0, 1}"),
    ("sdc_gae gamma=1.5", "sdc_gae: gamma = 1.500000 outside [0, 1]"),
    ("sdc_gae gamma=-0.25 gae_lambda=7", "sdc_gae: gamma = -0.250000 outside [0, 1]"),
    ("sdc_gae gamma=nan", "sdc_gae: gamma = nan outside [0, 1]"),
    ("sdc_gae gamma=inf", "sdc_gae: gamma = inf outside [0, 1]"),
    ("sdc_gae gae_lambda=1.25", "sdc_gae: gae_lambda = 1.250000 outside [0, 1]"),
    ("sdc_gae gae_lambda=-1", "sdc_gae: gae_lambda = -1.000000 outside [0, 1]"),
    ("sdc_gae gae_lambda=nan value_preds=%d" % 0x7f0000002000, "sdc_gae: gae_lambda = nan outside [0, 1]"),
    ("sdc_gae value_preds=%d" % 0x7f0000002000,
     "sdc_gae: value_preds asked for while no critic is set (sdc_set_critic first: its scale and shift)"),
    ("sdc_action_log_probs", None),
    ("sdc_action_log_probs entropy=0 n_steps=672", None),                                        # (entropy may be NULL)
    ("sdc_action_log_probs handle=0", "sdc_action_log_probs: null handle"),
    ("sdc_action_log_probs handle=0 n_steps=0", "sdc_action_log_probs: null handle"),
    ("sdc_action_log_probs n_steps=0", "sdc_action_log_probs: n_steps = 0 must be positive"),
    ("sdc_action_log_probs n_steps=-1 actions=0", "sdc_action_log_probs: n_steps = -1 must be positive"),
    *[("sdc_action_log_probs %s=0" % a, A_NULL) for a in ("actions", "logits", "log_probs")],
    ("sdc_action_log_probs logits=0 entropy=%d" % ODD, A_NULL),
    *[("sdc_action_log_probs %s=%d" % (a, ODD), A_ALIGN) for a in ("actions", "logits", "log_probs", "entropy")],
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
    return build_driver(tmp_path_factory.mktemp("onpolicy_refusals"), ["-O1"], "driver")


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
    for entry in ("sdc_gae", "sdc_action_log_probs"):
        assert any(r.split()[0] == entry and t is None for r, t in CASES) and any(r.split()[0] == entry and t for r, t in CASES)
    assert all(t.startswith(r.split()[0] + ": ") for r, t in CASES if t is not None)
    assert len(texts) == 23
