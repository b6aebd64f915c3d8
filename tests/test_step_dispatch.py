"""Which kernel a stepping call lands on (csrc/sdc_dispatch.hpp), without a GPU: the header compiled by g++ alone into a program that
reads fact records and prints the three decisions, held to
  * the tables the GPU tests verified on the device (tests/step_paths.py: KERNEL_OF_BATCH, expected_mapping over RACK_CASES, ROLLOUT_CASES),
  * answers written out here case by case from the documented rules (include/sustaindc_hip.h SDC_DEBUG_*),
  * and, over a grid of some thirty thousand records, a restatement of those rules in Python that shares no text with the header."""
import itertools
import subprocess

import pytest

from dc_rl_amd import _lib as L
from tests.step_paths import GENERAL, KERNEL_NAME, KERNEL_OF_BATCH, PAIR, QUAD, RACK_CASES, ROLLOUT_CASES, WIDE, WIDE_OFF, expected_mapping

VERIFY, STEP_NO_ENV, BOUND_REPAIR = L.DEBUG_VERIFY, L.DEBUG_STEP_NO_ENV, L.DEBUG_BOUND_REPAIR
MEASUREMENT = (L.DEBUG_WHY_REBUILD, L.DEBUG_PHASES, L.DEBUG_STAMPS, L.DEBUG_RECORD_WAIT, L.DEBUG_HW_ID)
NAMED = VERIFY | STEP_NO_ENV | BOUND_REPAIR | GENERAL | PAIR | QUAD | WIDE | WIDE_OFF | L.PLAN_DEBUG_TWO_STEPS | sum(MEASUREMENT)
FIELDS = ("n_envs", "n_cfg", "racks_cfg0", "rack_cls_cfg0", "racks_max", "prm_env_ok", "wide_gen_ok", "has_qcum_t", "has_feat",
          "n_feat_host", "rel_hint", "p0", "p1", "p2", "r0", "r1", "r2", "flags", "actions", "share_obs", "info", "actions_out", "timed",
          "rows_al16", "actions_out_al4")
MULTI_KERNEL = {"general": "sdc_rollout_kernel", "pair": "sdc_rollout_fast_kernel", "quad": "sdc_rollout_quad_kernel"}

DRIVER = r"""
#include <cstdio>
#include "sdc_dispatch.hpp"
static const char* NAMES[5] = {"general", "pair", "quad", "wide", "wide_gen"};
int main() {
  char tag;
  while (std::scanf(" %c", &tag) == 1) {
    if (tag == 'M') {      // mirrors: n_envs flags
      int n, fl;
      if (std::scanf("%d %d", &n, &fl) != 2) return 2;
      const SdcWideMirrors m = sdc_wide_mirrors(n, fl);
      std::printf("%d %d\n", (int)m.qcum_t, (int)m.hist_t);
    } else if (tag == 'K') {      // the kernel table: path kind n_envs
      int p, k, n;
      if (std::scanf("%d %d %d", &p, &k, &n) != 3) return 2;
      const SdcKernelInfo i = sdc_kernel_of((SdcStepPath)p, (SdcLaunchKind)k);
      std::printf("%s %d %d %d %d\n", i.name ? i.name : "-", i.envs_per_block, i.waves_per_block, (int)i.sweep, sdc_env_blocks(i, n));
    } else if (tag == 'F') {
      int v[25];
      for (int i = 0; i < 25; i++)
        if (std::scanf("%d", &v[i]) != 1) return 2;
      SdcStepFacts f;
      f.n_envs = v[0]; f.n_cfg = v[1]; f.racks_cfg0 = v[2]; f.rack_cls_cfg0 = v[3]; f.racks_max = v[4]; f.prm_env_ok = v[5];
      f.wide_gen_ok = v[6]; f.has_qcum_t = v[7]; f.has_feat = v[8]; f.n_feat_host = v[9]; f.rel_hint = v[10];
      for (int a = 0; a < 3; a++) { f.policy[a] = v[11 + a]; f.reward_method[a] = v[14 + a]; }
      f.debug_flags = v[17]; f.actions = v[18]; f.share_obs = v[19]; f.info = v[20]; f.actions_out = v[21]; f.timed = v[22];
      f.rows_al16 = v[23]; f.actions_out_al4 = v[24];
      const SdcStepPath s = sdc_single_step_path(f);
      const SdcRolloutPath r = sdc_rollout_path(f);
      const SdcActorPath a = sdc_actor_path(f);
      std::printf("%s %s | %s %d %s | %s\n", NAMES[s], sdc_kernel_of(s, SDC_LAUNCH_SINGLE).name, NAMES[r.path], (int)r.per_step,
                  sdc_kernel_of(r.path, r.per_step ? SDC_LAUNCH_SINGLE : SDC_LAUNCH_MULTI).name,
                  a.refused ? "refused" : sdc_kernel_of(a.path, SDC_LAUNCH_ACTOR).name);
    } else {
      return 3;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """the driver, built once by g++ alone (no HIP on the include path); -> a function from input lines to output lines"""
    d = tmp_path_factory.mktemp("dispatch")
    src, exe = d / "driver.cpp", str(d / "driver")
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + L.CSRC, str(src), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def has_mirror(n, flags):
    """what sdc_create gives a batch: the queue table's time-major mirror for multiples of 64 envs from 7680, or with WIDE"""
    return n % 64 == 0 and (n >= 7680 or bool(flags & WIDE))


def facts(n=256, flags=0, **kw):
    """a lock-step batch of one 20-rack config in the common case, as sdc_create and a reset leave it; then what the case changes"""
    f = dict(n_envs=n, n_cfg=1, racks_cfg0=20, rack_cls_cfg0=4, racks_max=20, prm_env_ok=0, wide_gen_ok=1, has_qcum_t=int(has_mirror(n, flags)),
             has_feat=1, n_feat_host=n, rel_hint=5, p0=0, p1=0, p2=0, r0=0, r1=0, r2=0, flags=flags, actions=1, share_obs=1, info=1,
             actions_out=0, timed=0, rows_al16=1, actions_out_al4=1)
    assert set(kw) <= set(f), kw
    f.update(kw)
    return f


def line(f):
    return "F " + " ".join(str(int(f[k])) for k in FIELDS)


def decide(ask, fs):
    """-> per record (single-step path, rollout (path, per_step, kernel), closed-loop kernel or "refused")"""
    out = []
    for ln in ask([line(f) for f in fs]):
        s, r, a = (part.split() for part in ln.split("|"))
        assert s[1] == KERNEL_NAME[s[0]]
        out.append((s[0], (r[0], bool(int(r[1])), r[2]), a[0]))
    return out


def test_header_compiles_without_hip_and_names_every_kernel(ask):
    """the table: kernel, envs and wavefronts per workgroup, who sweeps (0 nobody, 1 the workgroups sdc_create sized, 2 the lane-per-env
    kernel's own), workgroups that carry envs for a batch of 5636 / 7744 envs"""
    rows = [(0, 0, 5636, "sdc_dynamics_kernel", 8, 4, 1, 705), (1, 0, 5636, "sdc_dynamics_fast_kernel", 8, 4, 1, 705),
            (2, 0, 5636, "sdc_dynamics_quad_kernel", 16, 4, 1, 353), (3, 0, 7744, "sdc_dynamics_wide_kernel", 64, 2, 2, 121),
            (4, 0, 7744, "sdc_dynamics_wide_gen_kernel", 64, 2, 2, 121), (0, 1, 5635, "sdc_rollout_kernel", 8, 4, 0, 705),
            (1, 1, 5636, "sdc_rollout_fast_kernel", 8, 4, 0, 705), (2, 1, 5636, "sdc_rollout_quad_kernel", 16, 4, 0, 353),
            (1, 2, 5636, "sdc_rollout_actor_kernel", 16, 8, 0, 353), (2, 2, 5636, "sdc_rollout_actor_quad_kernel", 32, 8, 0, 177)]
    out = ask([f"K {p} {k} {n}" for p, k, n, *_ in rows])
    for (p, k, n, *want), got in zip(rows, out):
        assert got.split() == [str(w) for w in want], (p, k, got)
    # no multi-step or closed-loop form of the lane-per-env kernel, no closed loop on the general kernel
    assert [o.split()[0] for o in ask(["K 3 1 64", "K 4 1 64", "K 3 2 64", "K 4 2 64", "K 0 2 64"])] == ["-"] * 5


def test_single_steps_by_batch_size_land_where_the_device_tests_found_them(ask):
    sizes = sorted(KERNEL_OF_BATCH)
    got = decide(ask, [facts(n) for n in sizes])
    assert [g[0] for g in got] == [KERNEL_OF_BATCH[n] for n in sizes]
    assert [KERNEL_OF_BATCH[n] for n in sizes] == ["pair", "pair", "quad", "quad", "wide", "general", "pair", "quad", "wide", "wide", "wide"]


def test_rack_counts_and_classes_land_where_the_device_tests_found_them(ask):
    """tests/test_gpu_kernel_reach.py's 256-env batches: one config of the case's racks / classes, or two configs (20 racks beside it),
    under each forcing flag.  (A config of more than 8 classes has no class table: rack_cls_cfg0 = 0; more than 12: wide_gen_ok off.)"""
    fs, want = [], []
    for racks, classes in RACK_CASES:
        k = classes if classes is not None else min(racks, 4)
        for two in (False, True):
            for fl in ((GENERAL, WIDE) if two else (GENERAL, PAIR, QUAD, WIDE, WIDE_OFF)):
                fs.append(facts(256, fl, n_cfg=2 if two else 1, racks_cfg0=racks, racks_max=max(racks, 20) if two else racks,
                                rack_cls_cfg0=k if k <= 8 else 0, prm_env_ok=int(two), wide_gen_ok=int(k <= 12 and racks <= 32)))
                want.append(expected_mapping(fl, racks, k, two))
    assert [g[0] for g in decide(ask, fs)] == want


def test_one_condition_at_a_time_from_the_common_case(ask):
    base = decide(ask, [facts()])[0]
    assert base == ("pair", ("pair", False, "sdc_rollout_fast_kernel"), "sdc_rollout_actor_kernel")
    flips = {
        "out of lock-step": dict(rel_hint=-1), "an env without feature rows": dict(n_feat_host=255), "no feature rows at all": dict(has_feat=0),
        "info missing": dict(info=0), "share_obs missing": dict(share_obs=0), "33 racks": dict(racks_cfg0=33, racks_max=33),
        "no racks set": dict(racks_cfg0=0), "a policy on slot 0": dict(p0=1), "a policy on slot 1": dict(p1=3), "a policy on slot 2": dict(p2=2),
        "reward on slot 1": dict(r1=1), "reward on slot 2": dict(r2=3), "reward on slot 0": dict(r0=1),
        "the general kernel asked for": dict(flags=GENERAL), "the bound-repair hook": dict(flags=BOUND_REPAIR),
        "a bit without a name (2)": dict(flags=4), "a bit without a name (15)": dict(flags=1 << 15),
        **{f"measurement bit {b}": dict(flags=b) for b in MEASUREMENT},
    }
    got = decide(ask, [facts(**kw) for kw in flips.values()])
    for what, g in zip(flips, got):
        assert g == ("general", ("general", False, "sdc_rollout_kernel"), "refused"), what
    # a profiled step is sdc_step's alone
    assert decide(ask, [facts(timed=1)])[0][0] == "general"
    # an odd batch
    assert decide(ask, [facts(257)])[0] == ("general", ("general", False, "sdc_rollout_kernel"), "refused")
    # flags that do not touch the choice: verify mode (a launch of its own; the closed loop refuses it), sdc_create's hook
    assert decide(ask, [facts(flags=VERIFY)])[0] == ("pair", ("pair", False, "sdc_rollout_fast_kernel"), "refused")
    assert decide(ask, [facts(flags=STEP_NO_ENV)])[0] == base
    # several configs: the common case while every env has its own copy of the scalars and no config has more than 32 racks
    two = dict(n_cfg=2, prm_env_ok=1, racks_cfg0=33, racks_max=25)
    assert decide(ask, [facts(**two)])[0] == base
    assert decide(ask, [facts(**dict(two, prm_env_ok=0))])[0][0] == "general"
    assert decide(ask, [facts(**dict(two, racks_max=33))])[0][0] == "general"


def test_the_forced_lane_per_env_kernel_and_its_general_form(ask):
    one = lambda flags=WIDE, **kw: decide(ask, [facts(256, flags, **kw)])[0][0]
    assert one() == "wide"
    for kw in (dict(p0=1), dict(p2=2), dict(p0=1, p1=3, p2=2), dict(p0=1, p1=1, p2=2, actions=0), dict(r1=1), dict(r2=5), dict(r1=2, r2=2),
               dict(rack_cls_cfg0=0), dict(n_cfg=2, prm_env_ok=1, racks_max=25)):
        assert one(**kw) == "wide_gen", kw
        # ... and without the general form's tables: the common case on two envs per wavefront, anything else on the general kernel
        common = not any(kw.get(k) for k in ("p0", "p1", "p2", "r1", "r2"))
        assert one(wide_gen_ok=0, **kw) == ("pair" if common else "general"), kw
    assert one(r0=1) == "general"                                  # only default_ls_reward appends to the history
    assert one(p0=1, actions=0) == "general"                       # no actions, and not every slot has a policy
    for kw in (dict(info=0), dict(share_obs=0), dict(timed=1), dict(rel_hint=-1), dict(n_feat_host=3), dict(flags=WIDE | GENERAL),
               dict(flags=WIDE | L.DEBUG_PHASES), dict(racks_cfg0=33, racks_max=33, wide_gen_ok=0)):
        assert one(**kw) == "general", kw


def test_mapping_overrides(ask):
    one = lambda n, fl, **kw: decide(ask, [facts(n, fl, **kw)])[0][0]
    # two envs per wavefront beats size
    assert [one(n, PAIR) for n in (5636, 8192, 49152)] == ["pair"] * 3
    # four: a multiple of four envs of ONE config
    assert one(256, QUAD) == "quad" and one(258, QUAD) == "pair" and one(4, QUAD) == "quad"
    assert one(256, QUAD, n_cfg=2, prm_env_ok=1) == "pair" and one(8004, 0, n_cfg=2, prm_env_ok=1) == "pair"
    # one lane per env: a multiple of 64 envs, the queue table's mirror, 16-byte aligned rows
    assert one(256, WIDE) == "wide" and one(320, WIDE) == "wide" and one(64, WIDE) == "wide"
    assert one(288, WIDE) == "pair" and one(258, WIDE) == "pair"
    assert one(256, WIDE, has_qcum_t=0) == "pair" and one(8192, 0, has_qcum_t=0) == "quad"
    assert one(256, WIDE, rows_al16=0) == "pair" and one(8192, 0, rows_al16=0) == "quad" and one(8192 + 64 * 3 + 2, 0, rows_al16=0) == "pair"
    assert one(256, WIDE, rows_al16=0, p2=2) == "general"           # (the general form stores whole lines as well)
    # ... kept off
    assert one(8192, WIDE_OFF) == "quad" and one(8192, 0) == "wide" and one(256, WIDE | WIDE_OFF) == "pair"
    # another mapping asked for beside it: not the lane-per-env kernel
    assert one(256, PAIR | WIDE) == "pair" and one(256, QUAD | WIDE) == "quad" and one(8192, PAIR) == "pair" and one(8192, QUAD) == "quad"
    assert one(256, PAIR | WIDE, p2=2) == "general"                 # ... nor its general form
    # two beats four
    assert one(8192, PAIR | QUAD) == "pair"


def test_rollouts(ask):
    one = lambda n, fl=0, **kw: decide(ask, [facts(n, fl, **kw)])[0][1]
    assert one(4096) == ("pair", False, "sdc_rollout_fast_kernel")
    assert one(4098) == ("pair", False, "sdc_rollout_fast_kernel")
    assert one(4100) == ("quad", False, "sdc_rollout_quad_kernel")
    assert one(7680) == ("quad", False, "sdc_rollout_quad_kernel")        # single steps: one lane per env; a rollout: not yet
    assert one(12284) == ("quad", False, "sdc_rollout_quad_kernel")
    assert one(12288) == ("wide", True, "sdc_dynamics_wide_kernel")
    assert one(12288, WIDE_OFF) == ("quad", False, "sdc_rollout_quad_kernel")
    assert one(12288, rows_al16=0) == ("quad", False, "sdc_rollout_quad_kernel")
    # the applied actions wanted: only the general kernels write them
    assert one(12288, actions_out=1) == ("wide_gen", True, "sdc_dynamics_wide_gen_kernel")
    assert one(12288, actions_out=1, wide_gen_ok=0) == ("general", False, "sdc_rollout_kernel")
    assert one(12288, actions_out=1, actions_out_al4=0) == ("general", False, "sdc_rollout_kernel")
    for n in (256, 4096, 4100, 7680, 12284):
        assert one(n, actions_out=1) == ("general", False, "sdc_rollout_kernel"), n
    # no actions, a policy on every slot
    pol = dict(p0=1, p1=3, p2=2, actions=0)
    assert one(256, **pol) == one(7680, **pol) == ("general", False, "sdc_rollout_kernel")
    assert one(12288, **pol) == one(12288, actions_out=1, **pol) == ("wide_gen", True, "sdc_dynamics_wide_gen_kernel")
    assert one(12288, wide_gen_ok=0, **pol) == ("general", False, "sdc_rollout_kernel")
    # what the device tests found (K = 3 on small batches)
    got = decide(ask, [facts(n, fl, actions_out=int(ao)) for n, fl, ao, _ in ROLLOUT_CASES])
    assert [g[1][2] for g in got] == [c[3] for c in ROLLOUT_CASES]
    assert [g[1][1] for g in got] == [c[3].startswith("sdc_dynamics_wide") for c in ROLLOUT_CASES]


def test_closed_loop(ask):
    one = lambda n, fl=0, **kw: decide(ask, [facts(n, fl, **kw)])[0][2]
    pair, quad = "sdc_rollout_actor_kernel", "sdc_rollout_actor_quad_kernel"
    assert [one(n) for n in (2, 256, 4096, 4098, 4100, 4102, 8192, 49152)] == [pair, pair, pair, pair, quad, pair, quad, quad]
    assert one(256, QUAD) == quad and one(258, QUAD) == pair and one(8192, PAIR) == pair and one(8192, PAIR | QUAD) == pair
    assert one(256, WIDE) == pair and one(8192, WIDE) == quad and one(8192, WIDE_OFF) == quad      # (never one lane per env)
    assert one(4100, n_cfg=2, prm_env_ok=1) == pair
    for kw in (dict(n=257), dict(fl=VERIFY), dict(fl=GENERAL), dict(fl=L.DEBUG_PHASES), dict(rel_hint=-1), dict(n_feat_host=0), dict(p1=3),
               dict(r2=1), dict(racks_cfg0=33), dict(n_cfg=2, prm_env_ok=0), dict(share_obs=0), dict(info=0)):
        assert one(kw.pop("n", 256), kw.pop("fl", 0), **kw) == "refused", kw


def test_which_mirrors_a_batch_gets(ask):
    cases = [(7616, 0, "0 0"), (7680, 0, "1 0"), (7681, 0, "0 0"), (49088, 0, "1 0"), (49152, 0, "1 1"), (49216, 0, "1 1"), (256, 0, "0 0"),
             (256, WIDE, "1 0"), (258, WIDE, "0 0"), (256, WIDE | PAIR, "1 0"), (8192, WIDE_OFF, "1 0")]
    assert ask([f"M {n} {fl}" for n, fl, _ in cases]) == [c[2] for c in cases]
    assert all(has_mirror(n, fl) == (w[0] == "1") for n, fl, w in cases)


def restated(f):
    """The documented rules once more, for the grid below."""
    n, fl = f["n_envs"], f["flags"]
    pol, rew = (f["p0"], f["p1"], f["p2"]), (f["r0"], f["r1"], f["r2"])
    general_asked = bool(fl & (GENERAL | BOUND_REPAIR | sum(MEASUREMENT))) or bool(fl & ~NAMED)
    special = (f["rel_hint"] >= 0 and f["has_feat"] and f["n_feat_host"] == n and f["share_obs"] and f["info"] and not f["timed"]
               and n % 2 == 0 and not general_asked)
    racks = 0 < f["racks_cfg0"] <= 32 if f["n_cfg"] == 1 else (f["prm_env_ok"] and f["racks_max"] <= 32)
    common = bool(special and racks and f["actions"] and pol == (0, 0, 0) and rew == (0, 0, 0))
    lanes = bool(has_mirror(n, fl) and f["has_qcum_t"] and not fl & (PAIR | QUAD | WIDE_OFF) and f["rows_al16"])
    lanes_common = lanes and f["n_cfg"] == 1 and f["racks_cfg0"] <= 32 and f["rack_cls_cfg0"] > 0
    lanes_general = bool(special and lanes and f["wide_gen_ok"] and (f["actions"] or 0 not in pol) and rew[0] == 0)
    four = lambda frm: n % 4 == 0 and f["n_cfg"] == 1 and not fl & PAIR and (n >= frm or bool(fl & QUAD))
    if common and lanes_common:
        single = "wide"
    elif lanes_general:
        single = "wide_gen"
    else:
        single = ("quad" if four(5636) else "pair") if common else "general"
    plain = common and not f["actions_out"]
    if (n >= 12288 or fl & WIDE) and plain and lanes_common:
        roll = ("wide", True, KERNEL_NAME["wide"])
    elif (n >= 12288 or fl & WIDE) and lanes_general and (not f["actions_out"] or f["actions_out_al4"]):
        roll = ("wide_gen", True, KERNEL_NAME["wide_gen"])
    else:
        p = ("quad" if four(4100) else "pair") if plain else "general"
        roll = (p, False, MULTI_KERNEL[p])
    if not common or fl & VERIFY:
        actor = "refused"
    else:
        actor = "sdc_rollout_actor_quad_kernel" if four(4100) else "sdc_rollout_actor_kernel"
    return single, roll, actor


def test_a_grid_of_records_against_the_rules_restated(ask):
    sizes = (254, 256, 257, 258, 260, 320, 4096, 4100, 5632, 5636, 7680, 7684, 12284, 12288, 49152)
    flag_sets = (0, VERIFY, PAIR, QUAD, WIDE, WIDE_OFF, GENERAL, PAIR | WIDE, QUAD | WIDE, WIDE | WIDE_OFF, PAIR | QUAD, L.DEBUG_PHASES | WIDE, 4)
    configs = (dict(), dict(rack_cls_cfg0=0), dict(rack_cls_cfg0=0, wide_gen_ok=0), dict(n_cfg=2, prm_env_ok=1, racks_max=25),
               dict(racks_cfg0=33, racks_max=33, wide_gen_ok=0))
    agents = (dict(), dict(p2=2), dict(p0=1, p1=3, p2=2, actions=0), dict(r1=1), dict(r0=1))
    call = (dict(), dict(actions_out=1), dict(actions_out=1, actions_out_al4=0), dict(rows_al16=0), dict(info=0), dict(rel_hint=-1))
    fs = [facts(n, fl, **c, **a, **k) for n, fl, c, a, k in itertools.product(sizes, flag_sets, configs, agents, call)]
    got = decide(ask, fs)
    bad = [(f, g, restated(f)) for f, g in zip(fs, got) if g != restated(f)]
    assert not bad, (len(bad), bad[:3])
    assert {g[0] for g in got} == set(KERNEL_NAME) and {g[2] for g in got} == {"refused", "sdc_rollout_actor_kernel", "sdc_rollout_actor_quad_kernel"}
