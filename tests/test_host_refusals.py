"""What the C-ABI refuses and with which words (csrc/sdc_refusals.hpp), without a GPU: the header compiled by g++ alone into a program
that reads one request line per case and prints the rule's message, or `-` for a call it accepts.  The table of cases is
tests/refusal_cases.py -- every text a literal, none built by the code under test; the same table runs through the same program built
with -fsanitize=address,undefined.

A request line:  <entry point> key=value key=value ...   Every key has a default (the driver's, restated in tests/refusal_cases.py):
an engine of 8 envs and 96-step episodes that has been reset once, and the entry point's smallest legal arguments.
  the handle     handle started debug_flags all_policies actor_set=a,b,c actor_act=a,b,c latch critic n_envs T hist_cap n_loc n_cfg
                 auto_reset tables_set assigned has_feat layout qstride lw engine_id fc_mode=w,c,t,wb fc_entries fc_values racks
  the mirror     t_rel=[N] cfg_ids=[N] loc_ids=[N] nofeat=envs marked=1 (one mark of the whole batch, serial 1) killed=envs
  an address     a number (0: NULL); never followed.  A list the rule reads: comma-separated values, or `null`
Behind the message, after a tab, the by-products a case may ask about: overrun=envs (sdc_rewind_envs), k_max=n (the planner
evaluations), gamma=g (the plan calls' objective with its defaults)."""
import subprocess

import pytest

from dc_rl_amd import _lib as L
from tests import refusal_cases as RC

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <iostream>
#include <map>
#include <sstream>
#include "sdc_refusals.hpp"

static std::map<std::string, std::string> R;
static std::deque<std::vector<int32_t>> lists;
static std::deque<std::vector<double>> dlists;
static const long long GOOD = 0x7f0000001000ll;      // a made-up address, 4096-byte aligned
static const std::string* get(const char* k) {
  const auto it = R.find(k);
  return it == R.end() ? nullptr : &it->second;
}
static long long I(const char* k, const long long dflt) { return get(k) ? std::strtoll(get(k)->c_str(), nullptr, 0) : dflt; }
static double D(const char* k, const double dflt) { return get(k) ? std::strtod(get(k)->c_str(), nullptr) : dflt; }
template <class T>
static T* P(const char* k) { return reinterpret_cast<T*>((uintptr_t)I(k, GOOD)); }
// a list the rule reads: the key's values, or `dflt`; "null": NULL
static std::vector<int32_t>* V(const char* k, const std::vector<int32_t>& dflt) {
  if (get(k) && *get(k) == "null") return nullptr;
  lists.emplace_back(dflt);
  if (get(k)) {
    lists.back().clear();
    std::stringstream ss(*get(k));
    for (std::string x; std::getline(ss, x, ',');) lists.back().push_back((int32_t)std::strtoll(x.c_str(), nullptr, 0));
  }
  return &lists.back();
}
static int32_t* VP(const char* k, const std::vector<int32_t>& dflt) {
  std::vector<int32_t>* v = V(k, dflt);
  return v ? v->data() : nullptr;
}
static std::vector<double>& DV(const char* k) {
  dlists.emplace_back();
  if (get(k)) {
    std::stringstream ss(*get(k));
    for (std::string x; std::getline(ss, x, ',');) dlists.back().push_back(std::strtod(x.c_str(), nullptr));
  }
  return dlists.back();
}

static SdcHostMirror mirror;
static SdcCallFacts facts() {
  SdcCallFacts f;
  if (!I("handle", 1)) return f;
  f.handle = true;
  const int N = f.n_envs = (int)I("n_envs", 8);
  f.episode_steps = (int)I("T", 96);
  f.hist_cap = (int)I("hist_cap", 10000);
  f.n_locations = (int)I("n_loc", 1);
  f.n_dc_configs = (int)I("n_cfg", 1);
  f.auto_reset = (int)I("auto_reset", 0);
  f.debug_flags = (int)I("debug_flags", 0);
  f.all_policies = I("all_policies", 0) != 0;
  const std::vector<int32_t>&set = *V("actor_set", {0, 0, 0}), &act = *V("actor_act", {0, 0, 0});
  for (int a = 0; a < 3; a++) f.actor_set[a] = set[a] != 0, f.actor_activation[a] = act[a];
  f.latch_valid = I("latch", 0) != 0;
  f.critic_set = I("critic", 0) != 0;
  f.tables_set = I("tables_set", 1) != 0;
  f.assigned = I("assigned", 1) != 0;
  f.has_feat = I("has_feat", 1) != 0;
  f.state_layout = (uint32_t)I("layout", 0x1234);
  f.qstride = (int)I("qstride", 128);
  f.lw = (int)I("lw", 114);
  f.rec_dwords = 64;
  f.rec_cfg = 24;
  f.mark_engine_id = (int)I("engine_id", 0);
  const std::vector<int32_t>& mode = *V("fc_mode", {0, 0, 0, 0});
  for (int c = 0; c < 4; c++) f.forecast.mode[c] = mode[c];
  f.forecast.values_entries = (int)I("fc_entries", 0);
  f.forecast.values = reinterpret_cast<const double*>((uintptr_t)I("fc_values", 0));
  f.started = I("started", 1) != 0;
  mirror = SdcHostMirror(N, f.episode_steps, f.has_feat);
  if (f.started) mirror.reset(nullptr);
  if (get("t_rel")) mirror.reload_t_rel(VP("t_rel", {}));
  if (get("cfg_ids")) mirror.set_cfg_ids(VP("cfg_ids", {}));
  if (get("loc_ids")) mirror.set_loc_ids(VP("loc_ids", {}));
  for (const int e : *V("nofeat", {})) {
    const SdcEnvFacts x = {e, mirror.t_rel(e), false, mirror.cfg(e), mirror.loc(e)};
    mirror.replace_envs(&x, 1);
  }
  if (I("marked", 0)) mirror.mark(nullptr, N);
  for (const int e : *V("killed", {})) mirror.mark_kill(e);
  f.left = mirror.steps_to_terminal();
  f.mirror = &mirror;
  SdcStepFacts& s = f.step;      // the common case, but for what the keys change
  s.n_envs = N, s.n_cfg = f.n_dc_configs, s.racks_cfg0 = s.racks_max = (int)I("racks", 20), s.rack_cls_cfg0 = 7;
  s.wide_gen_ok = true, s.has_feat = f.has_feat, s.n_feat_host = mirror.n_feat(), s.rel_hint = mirror.rel_hint();
  for (int a = 0; a < 3; a++) s.policy[a] = SDC_POLICY_EXTERNAL, s.reward_method[a] = SDC_REWARD_DEFAULT;
  s.debug_flags = f.debug_flags;
  s.actions = s.share_obs = s.info = s.actions_out = s.rows_al16 = s.actions_out_al4 = true;
  return f;
}

static std::string by;      // the by-products, behind a tab
static void out(const char* m) { std::printf("%s%s%s\n", m ? m : "-", by.empty() ? "" : "\t", by.c_str()); }
static void out(const SdcMsg& m) { out(m ? m->c_str() : nullptr); }
static std::string join(const std::vector<int>& v) {
  std::string s;
  for (const int x : v) s += (s.empty() ? "" : ",") + std::to_string(x);
  return s;
}

static SdcStatsArrays stats_arrays() {
  return {P<double>("stats"), P<double>("returns"), P<int32_t>("counts"), P<float>("obs"), P<float>("share_obs"), P<float>("rew"),
          P<uint8_t>("done"), P<float>("info"), P<float>("final_obs")};
}
static sdc_plan_objective objective_;
static const sdc_plan_objective* objective() {
  if (!I("obj", 0)) return nullptr;
  sdc_plan_objective& o = objective_ = sdc_plan_objective{};
  o.reward_weight[0] = o.reward_weight[1] = o.reward_weight[2] = 1.0;
  o.gamma = D("gamma", 1.0);
  o.n_cols = (int)I("n_cols", 0);
  const std::vector<int32_t>& col = *V("col", {});
  for (size_t j = 0; j < col.size() && j < SDC_PLAN_MAX_COLS; j++) o.col[j] = col[j];
  return &o;
}
template <class Cem>
static void cem_common(Cem& c) {
  c.n_iters = (int)I("n_iters", 1), c.iter0 = (int)I("iter0", 0), c.n_elite = (int)I("n_elite", 1);
  const std::vector<int32_t>& fx = *V("fixed", {-1, -1, -1});
  for (int a = 0; a < 3; a++) c.fixed_action[a] = fx[a];
  c.alpha = D("alpha", 0.0), c.p_min = D("p_min", 0.0);
}
static sdc_cem_params cem() {
  sdc_cem_params c{};
  cem_common(c);
  c.n_cand = (int)I("n_cand", 2);
  return c;
}
static sdc_cem_group_params cem_groups() {
  sdc_cem_group_params c{};
  cem_common(c);
  c.group_size = (int)I("group_size", 2), c.group_base = (int)I("group_base", 0);
  return c;
}
template <class Mpc>
static void mpc_common(Mpc& m) {
  m.horizon = (int)I("horizon", 1), m.warm_start = (int)I("warm_start", 0), m.resume = (int)I("resume", 0);
  m.resume_steps = (int)I("resume_steps", 0);
  const std::vector<int32_t>& idle = *V("idle", {0, 0, 0});
  for (int k = 0; k < 3; k++) m.idle_action[k] = idle[k];
}

static bool answer(const std::string& e) {
  const SdcCallFacts f = facts();
  const int N = f.n_envs;
  const int n_steps = (int)I("n_steps", 1);
  const std::vector<int32_t> zeros((size_t)N, 0);
  by.clear();
  if (e == "sdc_set_tables") {
    out(sdc_set_tables_refused(f, (int)I("loc_id", 0), P<double>("W"), P<double>("C"), P<double>("T_"), P<double>("WB"), (int)I("n", 35040)));
  } else if (e == "sdc_set_dc_params") {
    out(sdc_set_dc_params_refused(f, (int)I("cfg_id", 0), P<sdc_dc_params>("p")));
  } else if (e == "sdc_assign_envs") {
    out(sdc_assign_envs_refused(f, VP("loc_id", zeros), VP("cfg_id", zeros), VP("day_lo", zeros), VP("day_hi", std::vector<int32_t>((size_t)N, 364))));
  } else if (e == "sdc_reset") {
    sdc_reset_override o{};
    o.day = VP("day", zeros), o.hour = VP("hour", zeros), o.roll_days = VP("roll", zeros);
    o.ci_min = P<double>("ci_min"), o.ci_max = P<double>("ci_max"), o.t_min = P<double>("t_min"), o.t_max = P<double>("t_max");
    o.t_win = P<double>("t_win"), o.wb_win = P<double>("wb_win");
    o.noise = reinterpret_cast<const double*>((uintptr_t)I("noise", 0));
    const std::vector<int32_t>* mask = V("mask", {});
    std::vector<uint8_t> m8;
    if (get("mask") && mask) m8.assign(mask->begin(), mask->end());
    out(sdc_reset_refused(f, get("mask") && mask ? m8.data() : nullptr, I("ovr", 0) ? &o : nullptr));
  } else if (e == "sdc_step") {
    out(sdc_step_refused(f, P<int32_t>("actions"), P<float>("obs"), P<float>("rew"), P<uint8_t>("done"), P<float>("info")));
  } else if (e == "sdc_rollout") {
    out(sdc_rollout_refused(f, n_steps, P<int32_t>("actions"), P<float>("obs"), P<float>("rew"), P<uint8_t>("done")));
  } else if (e == "sdc_set_actor") {
    static sdc_actor_params p;
    p.activation = (int)I("activation", 0);
    out(sdc_set_actor_refused(f, (int)I("slot", 0), I("p", 1) ? &p : nullptr));
  } else if (e == "sdc_rollout_actor") {
    out(sdc_rollout_actor_refused(f, f.step, n_steps, P<float>("obs"), P<float>("share_obs"), P<float>("rew"), P<uint8_t>("done"), P<float>("info"),
                                  P<int32_t>("actions_out")));
  } else if (e == "sdc_profile_enable") {
    out(sdc_profile_enable_refused(f));
  } else if (e == "sdc_profile_read") {
    out(sdc_profile_read_refused(f, P<double>("out5")));
  } else if (e == "sdc_get_state" || e == "sdc_set_state") {
    const bool named = !get("field") || *get("field") != "null";
    const std::string field = get("field") ? *get("field") : "day";
    const SdcFieldFacts fld = {(size_t)I("elem", 4), I("allocated", 1) != 0};
    const bool known = I("elem", 4) >= 0;
    std::vector<int32_t> buf = *V("ids", zeros);      // [N] config ids: the buffer itself, or the records' config dwords
    if (field == "record") {
      std::vector<int32_t> rec((size_t)N * 64, 0);
      for (int k = 0; k < N; k++) rec[(size_t)k * 64 + 24] = buf[(size_t)k];
      buf = rec;
    }
    const void* host = I("buf", 1) ? buf.data() : nullptr;
    const size_t bytes = (size_t)I("bytes", 4 * N);
    if (e == "sdc_get_state") out(sdc_get_state_refused(f, named ? field.c_str() : nullptr, host, bytes, known ? &fld : nullptr));
    else out(sdc_set_state_refused(f, named ? field.c_str() : nullptr, host, bytes, known ? &fld : nullptr));
  } else if (e == "sdc_clone_envs") {
    std::vector<int32_t>*src = V("src", {0}), *dst = V("dst", {1});
    std::vector<int> src_of;
    out(sdc_clone_envs_refused(f, src ? src->data() : nullptr, dst ? dst->data() : nullptr, (int)I("n", src ? (long long)src->size() : 1), src_of));
  } else if (e == "sdc_snapshot_envs") {
    std::vector<int32_t>* envs = V("envs", {0});
    out(sdc_snapshot_envs_refused(f, envs ? envs->data() : nullptr, (int)I("n", envs ? (long long)envs->size() : 1), P<void>("rows"),
                                  P<int32_t>("manifest"), P<float>("obs"), P<float>("share_obs")));
  } else if (e == "sdc_restore_envs") {
    std::vector<int32_t>*envs = V("envs", {0}), *idx = V("rows_idx", {0});
    std::vector<int> row_of;
    out(sdc_restore_envs_refused(f, idx ? idx->data() : nullptr, envs ? envs->data() : nullptr, (int)I("n", envs ? (long long)envs->size() : 1),
                                 P<void>("rows"), (int)I("n_rows", 1), VP("manifest", {}), P<float>("obs"), P<float>("share_obs"), row_of));
  } else if (e == "sdc_mark_envs") {
    std::vector<int32_t>* envs = get("envs") ? V("envs", {}) : nullptr;
    std::vector<int> row_of;
    out(sdc_mark_envs_refused(f, envs ? envs->data() : nullptr, (int)I("n", envs ? (long long)envs->size() : N), (int)I("max_steps", 1),
                              P<void>("rows"), P<int32_t>("manifest"), P<float>("obs"), P<float>("share_obs"), row_of));
  } else if (e == "sdc_rewind_envs") {
    std::vector<int32_t>* envs = get("envs") ? V("envs", {}) : nullptr;
    std::vector<int> row_of, overrun;
    const SdcMsg m = sdc_rewind_envs_refused(f, envs ? envs->data() : nullptr, (int)I("n", envs ? (long long)envs->size() : N), P<void>("rows"),
                                             VP("manifest", {}), P<float>("obs"), P<float>("share_obs"), row_of, overrun);
    by = "overrun=" + join(overrun);
    out(m);
  } else if (e == "sdc_set_plan_forecast") {
    sdc_plan_forecast fc{}, kept;
    const std::vector<int32_t>& mode = *V("mode", {0, 0, 0, 0});
    for (int c = 0; c < 4; c++) fc.mode[c] = mode[c];
    fc.values_entries = (int)I("entries", 0);
    fc.values = P<double>("values");
    out(sdc_set_plan_forecast_refused(f, I("fc", 1) ? &fc : nullptr, kept));
  } else if (e == "sdc_forecast_traces") {
    out(sdc_forecast_traces_refused(f, (int)I("n_entries", 1), (int)I("truth", 0), P<double>("out")));
  } else if (e == "sdc_plan") {
    sdc_plan_objective obj;
    const SdcMsg m = sdc_plan_refused(f, (int)I("n_cand", 1), n_steps, P<int32_t>("actions"), objective(), P<double>("score"), P<int32_t>("best"),
                                      P<int32_t>("best_action"), P<float>("obs"), P<float>("share_obs"), obj);
    if (!m) by = "gamma=" + std::to_string(obj.gamma);
    out(m);
  } else if (e == "sdc_set_plan_terms") {
    sdc_plan_terms t{}, kept;
    t.n_limits = (int)I("n_limits", 0), t.n_terminal = (int)I("n_terminal", 0);
    const std::vector<int32_t>&lc = *V("limit_col", {}), &ls = *V("limit_side", {}), &tc = *V("terminal_col", {});
    const std::vector<double>&lb = DV("limit_bound"), &lw = DV("limit_weight"), &tw = DV("terminal_weight");
    for (size_t j = 0; j < SDC_PLAN_MAX_LIMITS; j++) {
      if (j < lc.size()) t.limit_col[j] = lc[j];
      if (j < ls.size()) t.limit_side[j] = ls[j];
      if (j < lb.size()) t.limit_bound[j] = lb[j];
      if (j < lw.size()) t.limit_weight[j] = lw[j];
    }
    for (size_t j = 0; j < SDC_PLAN_MAX_TERMINAL; j++) {
      if (j < tc.size()) t.terminal_col[j] = tc[j];
      if (j < tw.size()) t.terminal_weight[j] = tw[j];
    }
    out(sdc_set_plan_terms_refused(f, I("terms", 1) ? &t : nullptr, kept));
  } else if (e == "sdc_set_critic") {
    static sdc_critic_params p;
    p.b3 = (float)D("b3", 0.0), p.scale = (float)D("scale", 1.0), p.shift = (float)D("shift", 0.0), p.flags = (int)I("flags", 0);
    out(sdc_set_critic_refused(f, I("p", 1) ? &p : nullptr));
  } else if (e == "sdc_critic_values") {
    out(sdc_critic_values_refused(f, P<float>("share_obs"), I("n_rows", 1), P<float>("values")));
  } else if (e == "sdc_set_plan_critic") {
    out(sdc_set_plan_critic_refused(f, D("weight", 0.0)));
  } else if (e == "sdc_plan_cem") {
    const sdc_cem_params c = cem();
    sdc_plan_objective obj;
    out(sdc_plan_cem_refused(f, n_steps, I("cem", 1) ? &c : nullptr, objective(), P<double>("probs"), P<int32_t>("best_seq"),
                             P<double>("best_score"), P<int32_t>("best_action"), P<int32_t>("cand"), P<double>("cand_score"), P<float>("obs"),
                             P<float>("share_obs"), obj));
  } else if (e == "sdc_plan_cem_groups") {
    const sdc_cem_group_params c = cem_groups();
    sdc_plan_objective obj;
    out(sdc_plan_cem_groups_refused(f, n_steps, I("cem", 1) ? &c : nullptr, objective(), P<double>("probs"), P<int32_t>("best_seq"),
                                    P<double>("best_score"), P<int32_t>("best_action"), P<int32_t>("step_actions"), P<int32_t>("cand"),
                                    P<double>("cand_score"), P<float>("obs"), P<float>("share_obs"), obj));
  } else if (e == "sdc_rollout_stats") {
    out(sdc_rollout_stats_refused(f, n_steps, P<int32_t>("actions"), (int)I("accumulate", 0), stats_arrays()));
  } else if (e == "sdc_rollout_actor_stats") {
    out(sdc_rollout_actor_stats_refused(f, n_steps, (int)I("sample", 0), (int)I("accumulate", 0), stats_arrays(),
                                        reinterpret_cast<const int32_t*>((uintptr_t)I("policy_counts", 0)),
                                        reinterpret_cast<const double*>((uintptr_t)I("policy_sums", 0))));
  } else if (e == "sdc_rollout_cem_stats") {
    sdc_mpc_params m{};
    mpc_common(m);
    m.cem = cem();
    sdc_plan_objective obj;
    int k_max = -1;
    const SdcMsg r = sdc_rollout_cem_stats_refused(f, n_steps, I("mpc", 1) ? &m : nullptr, objective(), (int)I("accumulate", 0), stats_arrays(),
                                                   reinterpret_cast<const int32_t*>((uintptr_t)I("plan_counts", 0)),
                                                   reinterpret_cast<const double*>((uintptr_t)I("plan_sums", 0)), P<double>("probs"),
                                                   P<int32_t>("best_seq"), P<double>("best_score"), P<int32_t>("best_action"), P<int32_t>("cand"),
                                                   P<double>("cand_score"), obj, k_max);
    if (!r) by = "k_max=" + std::to_string(k_max);
    out(r);
  } else if (e == "sdc_rollout_cem_groups_stats") {
    sdc_mpc_group_params m{};
    mpc_common(m);
    m.sync_first = (int)I("sync_first", 0);
    m.cem = cem_groups();
    sdc_plan_objective obj;
    int k_max = -1;
    const SdcMsg r = sdc_rollout_cem_groups_stats_refused(
        f, n_steps, I("mpc", 1) ? &m : nullptr, objective(), (int)I("accumulate", 0), stats_arrays(),
        reinterpret_cast<const int32_t*>((uintptr_t)I("plan_counts", 0)), reinterpret_cast<const double*>((uintptr_t)I("plan_sums", 0)),
        reinterpret_cast<const int32_t*>((uintptr_t)I("diverged", 0)), P<double>("probs"), P<int32_t>("best_seq"), P<double>("best_score"),
        P<int32_t>("best_action"), P<int32_t>("step_actions"), P<int32_t>("cand"), P<double>("cand_score"), obj, k_max);
    if (!r) by = "k_max=" + std::to_string(k_max);
    out(r);
  } else {
    return false;
  }
  return true;
}

int main() {
  for (std::string line; std::getline(std::cin, line);) {
    std::stringstream ss(line);
    std::string entry, kv;
    ss >> entry;
    R.clear(), lists.clear(), dlists.clear();
    while (ss >> kv) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) return 2;
      R[kv.substr(0, eq)] = kv.substr(eq + 1);
    }
    if (!answer(entry)) return 3;
  }
  return 0;
}
"""


def build_driver(d, flags, name):
    """the driver built by g++ alone (no HIP on the include path)"""
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + L.CSRC, str(src)] + flags + ["-o", exe], check=True)
    return exe


def ask(exe, cases):
    out = subprocess.run([exe], input="\n".join(RC.request_line(c) for c in cases) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, (exe, out.returncode, out.stderr[-2000:])
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    return [tuple(ln.split("\t")) if "\t" in ln else (ln, "") for ln in lines]


def check(answers, cases):
    wrong = []
    for c, (msg, by) in zip(cases, answers):
        if msg != ("-" if c.text is None else c.text) or (c.by is not None and c.by != by):
            wrong.append((RC.request_line(c), c.text, c.by, msg, by))
    assert not wrong, wrong[:5]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("refusals"), ["-O1"], "driver")


def test_every_case_of_the_table(plain):
    check(ask(plain, RC.CASES), RC.CASES)


def test_every_case_under_the_address_and_undefined_behaviour_sanitizers(plain, tmp_path):
    """a stand-alone program run on its own: nothing is loaded into Python"""
    san = build_driver(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "driver_san")
    answers = ask(san, RC.CASES)
    check(answers, RC.CASES)
    assert answers == ask(plain, RC.CASES)


def test_the_table_covers_what_it_says():
    """every entry point of the header has an acceptance with no key changed but the facts it needs, a refusal, and a case of two faults"""
    entries = {c.entry for c in RC.CASES}
    assert entries == set(RC.ENTRY_POINTS) and len(entries) == 30
    for e in RC.ENTRY_POINTS:
        mine = [c for c in RC.CASES if c.entry == e]
        assert any(c.text is None for c in mine), e
        assert any(c.text is not None for c in mine), e
        assert any(c.two_faults for c in mine) or e in RC.ONE_RULE, e
    texts = [c.text for c in RC.CASES if c.text is not None]
    assert all(t.startswith(c.entry + ": ") for c, t in ((c, c.text) for c in RC.CASES if c.text is not None)), "a text names its entry point"
    assert len(set(texts)) >= 300
