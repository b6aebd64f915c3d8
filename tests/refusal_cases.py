"""The table of what the C-ABI refuses (csrc/sdc_refusals.hpp): an entry point, what the library knows of the handle, the call's
arguments, and the answer -- None for a call that is accepted, else the full text, written out here and nowhere built by the code under
test.  tests/test_host_refusals.py runs the table through the header on any machine; tests/test_gpu_refusal_wiring.py makes the cases
marked `wire` through the raw library calls on the device.  A plain module, like tests/plan_util.py.

How the table is laid out: per entry point, in the order of the header --
  the acceptance with the smallest legal arguments (no key given: the defaults below), then every rule in the order it is asked;
  the boundaries (the last value a rule accepts next to the first it refuses);
  `two=True`: two faults in one call, the earlier rule's text expected -- the order is part of the interface.
The defaults are the driver's: an engine of N = 8 envs with T = 96-step episodes, one location, one config, no auto-reset, no actor, no
critic, no mark, no forecast, reset once (every env at episode step 0); every address the made-up GOOD (4096-byte aligned, never
followed).  `facts`: what differs about the handle; the other keys: what differs about the arguments."""

N, T = 8, 96
LAYOUT, HIST_CAP, QSTRIDE, LW = 0x1234, 10000, 128, 114
GOOD = 0x7f0000001000
ENTRY_POINTS = (
    "sdc_set_tables", "sdc_set_dc_params", "sdc_assign_envs", "sdc_reset", "sdc_step", "sdc_rollout", "sdc_set_actor", "sdc_rollout_actor",
    "sdc_profile_enable", "sdc_profile_read", "sdc_get_state", "sdc_set_state", "sdc_clone_envs", "sdc_snapshot_envs", "sdc_restore_envs",
    "sdc_mark_envs", "sdc_rewind_envs", "sdc_set_plan_forecast", "sdc_forecast_traces", "sdc_plan", "sdc_set_plan_terms", "sdc_critic_values",
    "sdc_set_plan_critic", "sdc_plan_cem", "sdc_plan_cem_groups", "sdc_rollout_stats", "sdc_rollout_actor_stats", "sdc_rollout_cem_stats",
    "sdc_rollout_cem_groups_stats", "sdc_set_critic")
ONE_RULE = ("sdc_profile_enable", "sdc_profile_read")      # (a single rule each: no pair to order)


class Case:
    def __init__(self, entry, text, facts, args, by, two, wire):
        self.entry, self.text, self.facts, self.args, self.by, self.two_faults = entry, text, dict(facts or {}), args, by, two
        # through the raw library call: the engine of the wiring test is the default handle, so a case that changes no fact can be made
        self.wire = (not self.facts) if wire is None else wire


CASES = []


def ok(entry, facts=None, by=None, wire=False, **args):
    CASES.append(Case(entry, None, facts, args, by, False, wire))


def no(entry, text, facts=None, by=None, two=False, wire=None, **args):
    CASES.append(Case(entry, entry + ": " + text, facts, args, by, two, wire))


def request_line(c):
    def fmt(v):
        if v is None:
            return "null"
        if isinstance(v, (list, tuple)):
            return ",".join(fmt(x) for x in v)
        return float(v).hex() if isinstance(v, float) and v == v and abs(v) != float("inf") else str(v)
    pairs = dict(c.facts, **c.args)
    return " ".join([c.entry] + [f"{k}={fmt(v)}" for k, v in pairs.items()])


def where(lst, **at):
    """lst with entries replaced: where([0] * 8, _3=5) -> entry 3 is 5"""
    out = list(lst)
    for k, v in at.items():
        out[int(k[1:])] = v
    return out


Z, D364 = [0] * N, [364] * N
ALL = lambda v: [v] * N

# ---- sdc_set_tables ------------------------------------------------------------------------------------------------------------------------
E = "sdc_set_tables"
ok(E)
no(E, "null argument", facts=dict(handle=0), wire=True)
no(E, "null argument", W=0)
no(E, "null argument", WB=0)
no(E, "loc_id out of range", loc_id=1)
no(E, "loc_id out of range", loc_id=-1)
ok(E, facts=dict(n_loc=2), loc_id=1)
no(E, "tables must hold 35040 samples", n=35039)
no(E, "null argument", two=True, C=0, loc_id=5)
no(E, "loc_id out of range", two=True, loc_id=5, n=1)

# ---- sdc_set_dc_params -----------------------------------------------------------------------------------------------------------------------
E = "sdc_set_dc_params"
ok(E)
no(E, "null argument", facts=dict(handle=0), wire=True)
no(E, "null argument", p=0)
no(E, "cfg_id out of range", cfg_id=1)
no(E, "cfg_id out of range", cfg_id=-1)
no(E, "null argument", two=True, p=0, cfg_id=7)

# ---- sdc_assign_envs ---------------------------------------------------------------------------------------------------------------------
E = "sdc_assign_envs"
ok(E)
no(E, "null argument", facts=dict(handle=0), wire=True)
no(E, "null argument", day_hi=None)
no(E, "loc_id out of range", loc_id=where(Z, _3=1))
no(E, "cfg_id out of range", cfg_id=where(Z, _0=-1))
no(E, "bad day range", day_lo=where(Z, _7=-1))
no(E, "bad day range", day_hi=where(D364, _2=365))
no(E, "bad day range", day_lo=where(Z, _1=200), day_hi=where(D364, _1=199))
ok(E, day_lo=where(Z, _1=200), day_hi=where(D364, _1=200))
no(E, "loc_id out of range", two=True, loc_id=where(Z, _2=1), cfg_id=where(Z, _2=1))
no(E, "bad day range", two=True, day_lo=where(Z, _0=-1), loc_id=where(Z, _1=1))      # (env by env: env 0's day before env 1's location)

# ---- sdc_reset -----------------------------------------------------------------------------------------------------------------------------
E = "sdc_reset"
ok(E)
ok(E, mask=where(Z, _2=1))
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "call sdc_set_tables / sdc_set_dc_params / sdc_assign_envs first", facts=dict(tables_set=0))
no(E, "call sdc_set_tables / sdc_set_dc_params / sdc_assign_envs first", facts=dict(assigned=0))
ok(E, ovr=1, noise=GOOD)
no(E, "noise injection needs day, hour and roll_days", ovr=1, noise=GOOD, roll=None)
no(E, "noise injection needs day, hour and roll_days", ovr=1, noise=GOOD, day=None)
no(E, "injected day / hour / roll_days out of range", ovr=1, noise=GOOD, day=where(Z, _2=365))
no(E, "injected day / hour / roll_days out of range", ovr=1, noise=GOOD, hour=where(Z, _7=24))
no(E, "injected day / hour / roll_days out of range", ovr=1, noise=GOOD, roll=where(Z, _0=-1))
ok(E, ovr=1, noise=GOOD, day=ALL(364), hour=ALL(23), roll=ALL(364))
ok(E, ovr=1, noise=GOOD, day=where(Z, _2=365), mask=where([1] * N, _2=0))      # (an env that is not reset is not checked)
ok(E, ovr=1)
no(E, "incomplete override", ovr=1, ci_min=0)
no(E, "incomplete override", ovr=1, wb_win=0)
no(E, "incomplete override", ovr=1, hour=None)
no(E, "override day/hour out of range", ovr=1, hour=where(Z, _1=24))
no(E, "override day/hour out of range", ovr=1, day=where(Z, _5=-1))
ok(E, ovr=1, hour=where(Z, _1=24), mask=where(Z, _0=1))
no(E, "call sdc_set_tables / sdc_set_dc_params / sdc_assign_envs first", facts=dict(tables_set=0), two=True, ovr=1, t_max=0)
no(E, "noise injection needs day, hour and roll_days", two=True, ovr=1, noise=GOOD, hour=None, day=where(Z, _0=400))
no(E, "incomplete override", two=True, ovr=1, t_win=0, day=where(Z, _0=400))

# ---- sdc_step ------------------------------------------------------------------------------------------------------------------------------
E = "sdc_step"
ok(E)
no(E, "null argument", facts=dict(handle=0), wire=True)
no(E, "null argument", obs=0)
no(E, "null argument", rew=0)
no(E, "null argument", done=0)
no(E, "actions may only be NULL when every agent slot has a policy", actions=0)
ok(E, facts=dict(all_policies=1), actions=0)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "an environment has finished its episode; call sdc_reset (auto_reset is off)", facts=dict(t_rel=where(Z, _4=T)))
ok(E, facts=dict(t_rel=where(Z, _4=T - 1)))
ok(E, share_obs=0, info=0, final_obs=0)      # (the optional outputs)
no(E, "verify mode reports through info; info may not be NULL", facts=dict(debug_flags=1), info=0)
ok(E, facts=dict(debug_flags=1))
ok(E, facts=dict(debug_flags=2), info=0)      # (another bit: info stays optional)
no(E, "an environment has finished its episode; call sdc_reset (auto_reset is off)", facts=dict(debug_flags=1, t_rel=where(Z, _4=T)), two=True, info=0)
no(E, "null argument", two=True, done=0, actions=0)
no(E, "actions may only be NULL when every agent slot has a policy", facts=dict(started=0), two=True, actions=0)
no(E, "sdc_reset must be called first", facts=dict(started=0, t_rel=ALL(T)), two=True)

# ---- sdc_rollout ---------------------------------------------------------------------------------------------------------------------------
E = "sdc_rollout"
ok(E)
no(E, "null argument", facts=dict(handle=0), wire=True)
no(E, "null argument", rew=0)
no(E, "actions may only be NULL when every agent slot has a policy", actions=0)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "n_steps must be positive", n_steps=0)
no(E, "n_steps must be positive", n_steps=-3)
ok(E, n_steps=T)
no(E, "the rollout would run past the end of an episode (96 steps left); split it there", n_steps=T + 1)
no(E, "the rollout would run past the end of an episode (6 steps left); split it there", facts=dict(t_rel=where(Z, _1=90)), n_steps=7)
no(E, "verify mode checks single steps; use sdc_step", facts=dict(debug_flags=1))
no(E, "null argument", two=True, obs=0, n_steps=0)
no(E, "sdc_reset must be called first", facts=dict(started=0), two=True, n_steps=0)
no(E, "n_steps must be positive", facts=dict(debug_flags=1), two=True, n_steps=0)
no(E, "the rollout would run past the end of an episode (96 steps left); split it there", facts=dict(debug_flags=1), two=True, n_steps=97)

# ---- sdc_set_actor -----------------------------------------------------------------------------------------------------------------------
E = "sdc_set_actor"
ok(E)
ok(E, slot=2, activation=1)
no(E, "null argument", facts=dict(handle=0), wire=True)
no(E, "null argument", p=0)
no(E, "agent_slot must be 0 (ls), 1 (dc) or 2 (bat)", slot=3)
no(E, "agent_slot must be 0 (ls), 1 (dc) or 2 (bat)", slot=-1)
no(E, "activation must be 0 (tanh) or 1 (relu)", activation=2)
no(E, "activation must be 0 (tanh) or 1 (relu)", activation=-1)
no(E, "null argument", two=True, p=0, slot=3)
no(E, "agent_slot must be 0 (ls), 1 (dc) or 2 (bat)", two=True, slot=3, activation=2)

# ---- sdc_rollout_actor -----------------------------------------------------------------------------------------------------------------
E = "sdc_rollout_actor"
ACT = dict(actor_set=[1, 1, 1], latch=1)
COMMON_CASE = ("needs the common case (lock-step batch with feature rows, one data-centre config of <= 32 racks, external-action slots, "
               "default rewards, an even number of envs, no debug flags)")
ONE_ACTIVATION = "the three actors must share one activation (the reference builds them from one model config: happo.yaml activation_func)"
NO_OBS = "no observations yet (the actors were set after the last reset / step: reset or step once)"
ok(E, facts=ACT)
ok(E, facts=dict(ACT, actor_act=[1, 1, 1]), n_steps=T)
no(E, "null argument", facts=dict(handle=0), wire=True)
no(E, "null argument", facts=ACT, info=0)
no(E, "null argument", facts=ACT, actions_out=0)
no(E, "null argument", facts=ACT, share_obs=0)
no(E, "sdc_set_actor all three agents first")
no(E, "sdc_set_actor all three agents first", facts=dict(ACT, actor_set=[1, 0, 1]))
no(E, ONE_ACTIVATION, facts=dict(ACT, actor_act=[0, 1, 0]))
no(E, ONE_ACTIVATION, facts=dict(ACT, actor_act=[1, 1, 0]))
no(E, "sdc_reset must be called first", facts=dict(ACT, started=0))
no(E, NO_OBS, facts=dict(ACT, latch=0))
no(E, "n_steps must be positive", facts=ACT, n_steps=0)
no(E, "the rollout would run past the end of an episode (96 steps left); split it there", facts=ACT, n_steps=T + 1)
no(E, COMMON_CASE, facts=dict(ACT, racks=40))
no(E, COMMON_CASE, facts=dict(ACT, debug_flags=1))
no(E, COMMON_CASE, facts=dict(ACT, t_rel=where(Z, _3=2)))      # (not in lock-step)
no(E, COMMON_CASE, facts=dict(ACT, nofeat=[5]))
no(E, "null argument", two=True, info=0)      # (before the actors are asked about)
no(E, "sdc_set_actor all three agents first", two=True, n_steps=0)
no(E, ONE_ACTIVATION, facts=dict(ACT, actor_act=[0, 1, 0], started=0), two=True)
no(E, NO_OBS, facts=dict(ACT, latch=0), two=True, n_steps=0)
no(E, "the rollout would run past the end of an episode (96 steps left); split it there", facts=dict(ACT, racks=40), two=True, n_steps=97)

# ---- sdc_profile_enable, sdc_profile_read --------------------------------------------------------------------------------------------------
ok("sdc_profile_enable")
no("sdc_profile_enable", "null handle", facts=dict(handle=0), wire=True)
ok("sdc_profile_read")
no("sdc_profile_read", "null argument", facts=dict(handle=0), wire=True)
no("sdc_profile_read", "null argument", out5=0)

# ---- sdc_get_state, sdc_set_state ----------------------------------------------------------------------------------------------------------
# (field: a name of the library's table, `elem` bytes per env; elem=-1: no such field; allocated=0: an array this batch does not have)
E = "sdc_get_state"
ok(E)
no(E, "null argument", facts=dict(handle=0), wire=True)
no(E, "null argument", field=None)
no(E, "null argument", buf=0)
no(E, "unknown field nope", field="nope", elem=-1)
no(E, "size mismatch for day", bytes=31)
no(E, "size mismatch for day", bytes=33)
no(E, "this batch has no qcum_t", field="qcum_t", elem=512, bytes=4096, allocated=0)
no(E, "this batch has no hist_t", field="hist_t", elem=40000, bytes=320000, allocated=0)
ok(E, field="qcum_t", elem=512, bytes=4096, wire=False)
no(E, "null argument", two=True, buf=0, field="nope", elem=-1)
no(E, "unknown field nope", two=True, field="nope", elem=-1, bytes=1)
no(E, "size mismatch for qcum_t", two=True, field="qcum_t", elem=512, bytes=4, allocated=0)
E = "sdc_set_state"
ok(E)
no(E, "null argument", facts=dict(handle=0), wire=True)
no(E, "null argument", buf=0)
no(E, "unknown field nope", field="nope", elem=-1)
no(E, "qcum_t is derived from qtab: write that", field="qcum_t", elem=512, bytes=4096, wire=False)
no(E, "hist_t is derived from hist: write that", field="hist_t", elem=40000, bytes=320000, wire=False)
no(E, "size mismatch for day", bytes=8)
no(E, "cfg_id out of range", field="cfg_id", ids=where(Z, _6=1))
no(E, "cfg_id out of range", field="cfg_id", ids=where(Z, _0=-1))
ok(E, facts=dict(n_cfg=2), field="cfg_id", ids=where(Z, _6=1))
no(E, "record with a cfg_id out of range", field="record", elem=256, bytes=2048, ids=where(Z, _7=3))
ok(E, field="record", elem=256, bytes=2048)
no(E, "qcum_t is derived from qtab: write that", two=True, field="qcum_t", elem=512, bytes=1, wire=False)
no(E, "size mismatch for cfg_id", two=True, field="cfg_id", bytes=28, ids=where(Z, _0=5))

# ---- sdc_clone_envs ------------------------------------------------------------------------------------------------------------------------
E = "sdc_clone_envs"
ok(E)
ok(E, src=[0, 0, 3], dst=[1, 2, 7])
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "n must be positive", n=0)
no(E, "null index array", src=None, n=1)
no(E, "null index array", dst=None)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "pair 0 (0 -> 8) has an env index outside [0, 8)", dst=[8])
no(E, "pair 1 (-1 -> 2) has an env index outside [0, 8)", src=[0, -1], dst=[1, 2])
no(E, "dst 2 appears twice", src=[0, 1], dst=[2, 2])
no(E, "env 1 is both a src and a dst", src=[0, 1], dst=[1, 2])
no(E, "env 0 is both a src and a dst", src=[0], dst=[0])
no(E, "n must be positive", two=True, src=None, n=0)
no(E, "null index array", facts=dict(started=0), two=True, dst=None)
no(E, "pair 2 (9 -> 3) has an env index outside [0, 8)", two=True, src=[0, 0, 9], dst=[1, 1, 3])
no(E, "dst 2 appears twice", two=True, src=[2, 1], dst=[2, 2])

# ---- sdc_snapshot_envs ---------------------------------------------------------------------------------------------------------------------
E = "sdc_snapshot_envs"
ok(E)
ok(E, envs=[1, 1, 7])      # (an env may appear twice)
ok(E, envs=list(range(N)))
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "n must be positive", n=0)
no(E, "null array", envs=None, n=1)
no(E, "null array", manifest=0)
no(E, "null array", share_obs=0)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "n = 9 is more than the batch's 8 envs", envs=[0] * 9)
no(E, "env 8 (entry 0) outside [0, 8)", envs=[8])
no(E, "env -2 (entry 1) outside [0, 8)", envs=[3, -2])
ok(E, rows=GOOD + 256)
no(E, "rows must be 256-byte aligned", rows=GOOD + 128)
no(E, "n must be positive", two=True, n=0, rows=0)
no(E, "n = 9 is more than the batch's 8 envs", two=True, envs=[9] * 9)
no(E, "env 8 (entry 0) outside [0, 8)", two=True, envs=[8], rows=GOOD + 16)

# ---- sdc_restore_envs ----------------------------------------------------------------------------------------------------------------------
E = "sdc_restore_envs"


def snap_row(layout=LAYOUT, episode_steps=T, hist_cap=HIST_CAP, qstride=QSTRIDE, lw=LW, t_rel=0, feat=1, cfg=0, loc=0):
    return [layout, episode_steps, hist_cap, qstride, lw, t_rel, feat, cfg, loc]


ok(E, manifest=snap_row())
ok(E, manifest=snap_row() + snap_row(t_rel=T, feat=0), envs=[5, 2], rows_idx=[1, 0], n_rows=2)
no(E, "null handle", facts=dict(handle=0), wire=True, manifest=snap_row())
no(E, "n must be positive", manifest=snap_row(), n=0)
no(E, "n_rows must be positive", manifest=snap_row(), n_rows=0)
no(E, "null array", manifest=None)
no(E, "null array", manifest=snap_row(), rows_idx=None)
no(E, "null array", manifest=snap_row(), obs=0)
no(E, "sdc_reset must be called first", facts=dict(started=0), manifest=snap_row())
no(E, "env 8 (entry 0) outside [0, 8)", manifest=snap_row(), envs=[8])
no(E, "row 1 (entry 0) outside [0, 1)", manifest=snap_row(), rows_idx=[1])
no(E, "dst 2 appears twice", manifest=snap_row(), envs=[2, 2], rows_idx=[0, 0])
no(E, "row 0: state layout 4661, this engine's is 4660", manifest=snap_row(layout=LAYOUT + 1), wire=False)
no(E, "row 0: episode_steps 48, this engine's is 96", manifest=snap_row(episode_steps=48), wire=False)
no(E, "row 0: hist_cap 5, this engine's is 10000", manifest=snap_row(hist_cap=5), wire=False)
no(E, "row 0: queue stride 64, this engine's is 128", manifest=snap_row(qstride=64), wire=False)
no(E, "row 0: weather window length 66, this engine's is 114", manifest=snap_row(lw=66), wire=False)
no(E, "row 0: episode step 97 outside [0, episode_steps]", manifest=snap_row(t_rel=T + 1), wire=False)
no(E, "row 0: episode step -1 outside [0, episode_steps]", manifest=snap_row(t_rel=-1), wire=False)
no(E, "row 0: feature-rows flag 2", manifest=snap_row(feat=2), wire=False)
no(E, "row 0: cfg_id 1, this engine has 1 dc configs", manifest=snap_row(cfg=1), wire=False)
no(E, "row 0: loc_id -1, this engine has 1 locations", manifest=snap_row(loc=-1), wire=False)
no(E, "row 1: hist_cap 7, this engine's is 10000", manifest=snap_row() + snap_row(hist_cap=7), envs=[3], rows_idx=[1], n_rows=2, wire=False)
no(E, "rows must be 256-byte aligned", manifest=snap_row(), rows=GOOD + 128, wire=False)
no(E, "n must be positive", two=True, manifest=snap_row(), n=0, n_rows=0)
no(E, "n_rows must be positive", two=True, manifest=None, n_rows=0)
no(E, "env 9 (entry 1) outside [0, 8)", two=True, manifest=snap_row(), envs=[2, 9, 2], rows_idx=[0, 0, 0])
no(E, "row 0: cfg_id 4, this engine has 1 dc configs", two=True, manifest=snap_row(cfg=4, loc=4), rows=GOOD + 128, wire=False)

# ---- sdc_mark_envs -------------------------------------------------------------------------------------------------------------------------
E = "sdc_mark_envs"
ok(E)
ok(E, envs=[6, 1], max_steps=256)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "max_steps = 0 outside [1, 256]", max_steps=0)
no(E, "max_steps = 257 outside [1, 256]", max_steps=257)
no(E, "n must be positive", n=0)
no(E, "null array", rows=0)
no(E, "null array", manifest=0)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "n = 9 is more than the batch's 8 envs", envs=[0] * 9)
no(E, "envs == NULL means the whole batch: n must be 8, not 4", n=4)
no(E, "env -1 (entry 0) outside [0, 8)", envs=[-1])
no(E, "rows must be 256-byte aligned", rows=GOOD + 64)
no(E, "env 1 appears twice", envs=[1, 4, 1])
no(E, "max_steps = 0 outside [1, 256]", two=True, max_steps=0, n=0)
no(E, "n must be positive", facts=dict(started=0), two=True, n=0)
no(E, "rows must be 256-byte aligned", two=True, envs=[1, 1], rows=GOOD + 64)

# ---- sdc_rewind_envs -----------------------------------------------------------------------------------------------------------------------
E = "sdc_rewind_envs"
MARKED = dict(engine_id=7, marked=1)      # (one mark of the whole batch: serial 1)
DEAD = ("the mark is dead (a later mark of the env, a reset, sdc_set_state, a clone or restore into the env, or an earlier rewind refused "
        "beyond its max_steps)")


def mark_rows(envs=range(N), at=None, **kw):
    """the manifest rows of a mark of `envs` taken at episode step 0 with max_steps = 4; at={k: {field: value}} changes row k"""
    rows = []
    for k, e in enumerate(envs):
        r = dict(layout=LAYOUT, engine=7, steps=4, env=e, serial=1, t_rel=0, hist_cap=HIST_CAP)
        r.update(kw)
        r.update((at or {}).get(k, {}))
        rows += [r[f] for f in ("layout", "engine", "steps", "env", "serial", "t_rel", "hist_cap")]
    return rows


ok(E, facts=MARKED, by="overrun=", manifest=mark_rows())
ok(E, facts=dict(MARKED, t_rel=ALL(4)), by="overrun=", manifest=mark_rows([3, 5]), envs=[3, 5])      # (max_steps steps taken: still in reach)
no(E, "null handle", facts=dict(handle=0), wire=True, manifest=mark_rows())
no(E, "n must be positive", manifest=mark_rows(), n=0)
no(E, "null array", manifest=None)
no(E, "null array", manifest=mark_rows(), share_obs=0)
no(E, "sdc_reset must be called first", facts=dict(started=0), manifest=mark_rows())
no(E, "n = 9 is more than the batch's 8 envs", manifest=mark_rows(), n=9)
no(E, "envs == NULL means the whole batch: n must be 8, not 4", manifest=mark_rows(), n=4)
no(E, "env 8 (entry 0) outside [0, 8)", manifest=mark_rows([8]), envs=[8])
no(E, "rows must be 256-byte aligned", manifest=mark_rows(), rows=GOOD + 8)
no(E, "manifest with max_steps = 0 outside [1, 256]", manifest=mark_rows(steps=0), wire=False)
no(E, "manifest with max_steps = 257 outside [1, 256]", manifest=mark_rows(steps=257), wire=False)
no(E, "row 1 (env 1): state layout 4661, this library's is 4660", facts=MARKED, manifest=mark_rows(at={1: dict(layout=LAYOUT + 1)}))
no(E, "row 0 (env 0): the mark was taken from another engine (a mark goes back into the engine and the env it came from)", facts=MARKED,
   manifest=mark_rows(engine=8))
no(E, "row 0 (env 0): the mark was taken from another engine (a mark goes back into the engine and the env it came from)",
   facts=dict(MARKED, engine_id=0), manifest=mark_rows(engine=0))      # (an engine that has taken no mark)
no(E, "row 0 (env 3): the mark was taken from env 2", facts=MARKED, manifest=mark_rows([2]), envs=[3])
no(E, "row 1 (env 1): max_steps / hist_cap differ from the first row's / this engine's (the rows of a call come from one sdc_mark_envs call)",
   facts=MARKED, manifest=mark_rows(at={1: dict(steps=5)}))
no(E, "row 0 (env 0): max_steps / hist_cap differ from the first row's / this engine's (the rows of a call come from one sdc_mark_envs call)",
   facts=MARKED, manifest=mark_rows(hist_cap=9999))
no(E, "row 1 (env 2): the env appears twice", facts=MARKED, manifest=mark_rows([2, 2]), envs=[2, 2])
no(E, "row 0 (env 0): " + DEAD, facts=dict(MARKED, killed=[0]), manifest=mark_rows())
no(E, "row 0 (env 0): " + DEAD, facts=dict(engine_id=7), manifest=mark_rows())      # (no mark at all)
no(E, "row 2 (env 2): " + DEAD, facts=MARKED, manifest=mark_rows(at={2: dict(serial=2)}))
no(E, "row 0 (env 0): the env is at episode step 0, before the mark's 5", facts=MARKED, manifest=mark_rows(t_rel=5))
no(E, "row 0 (env 0): 10 steps taken since the mark, more than its max_steps = 4 (the mark is dead for good: slots beyond its reach have "
      "been overwritten)", facts=dict(MARKED, t_rel=ALL(10)), by="overrun=0,1,2,3,4,5,6,7", manifest=mark_rows())
no(E, "row 0 (env 4): 5 steps taken since the mark, more than its max_steps = 4 (the mark is dead for good: slots beyond its reach have "
      "been overwritten)", facts=dict(MARKED, t_rel=ALL(5)), by="overrun=4", manifest=mark_rows([4]), envs=[4])
no(E, "n must be positive", two=True, manifest=None, n=0)
no(E, "rows must be 256-byte aligned", two=True, manifest=mark_rows(steps=0), rows=GOOD + 8)
no(E, "manifest with max_steps = 0 outside [1, 256]", facts=MARKED, two=True, manifest=mark_rows(steps=0, layout=1), wire=False)
# (the scan goes on behind the first refusal: row 0 is named, and row 1's mark, which has been overrun, is reported for killing)
no(E, "row 0 (env 0): " + DEAD, facts=dict(MARKED, killed=[0], t_rel=where(Z, _1=9)), by="overrun=1", two=True, manifest=mark_rows())
no(E, "row 0 (env 0): state layout 1, this library's is 4660", facts=MARKED, two=True, manifest=mark_rows(at={0: dict(layout=1, engine=9)}))

# ---- sdc_set_plan_forecast -----------------------------------------------------------------------------------------------------------------
E = "sdc_set_plan_forecast"
ok(E)
ok(E, fc=0)
ok(E, mode=[3, 3, 3, 3], entries=0, values=0)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "mode[1] = 4 outside [0, 3]", mode=[0, 4, 0, 0])
no(E, "mode[3] = -1 outside [0, 3]", mode=[0, 0, 0, -1])
no(E, "values_entries = -1 is negative", entries=-1)
no(E, "mode[0] = 7 outside [0, 3]", two=True, mode=[7, 9, 0, 0], entries=-1)

# ---- sdc_forecast_traces -------------------------------------------------------------------------------------------------------------------
E = "sdc_forecast_traces"
VALUES = dict(fc_mode=[0, 3, 0, 0], fc_values=GOOD)      # (the carbon channel reads the caller's values)
ok(E)
ok(E, n_entries=T + 2)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "n_entries = 0 outside [1, 258]", n_entries=0)
no(E, "n_entries = 259 outside [1, 258]", n_entries=259)
no(E, "null out", out=0)
ok(E, out=GOOD + 8)
no(E, "out not 8-byte aligned", out=GOOD + 4)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "n_entries = 99 reaches past the end of an episode (96 steps left: at most that + 2 entries)", n_entries=T + 3)
no(E, "forecast channel 1 is SDC_FORECAST_VALUES and values is null", facts=dict(VALUES, fc_values=0, fc_entries=9))
no(E, "the forecast's values hold 2 entries, 3 are needed (n_steps + 2 at a plan call)", facts=dict(VALUES, fc_entries=2), n_entries=3)
ok(E, facts=dict(VALUES, fc_entries=3), n_entries=3)
ok(E, facts=dict(VALUES, fc_entries=2), n_entries=3, truth=1)      # (the truth reads no forecast)
no(E, "n_entries = 0 outside [1, 258]", two=True, n_entries=0, out=0)
no(E, "null out", facts=dict(started=0), two=True, out=0)
no(E, "out not 8-byte aligned", facts=dict(started=0), two=True, out=GOOD + 4)
no(E, "n_entries = 99 reaches past the end of an episode (96 steps left: at most that + 2 entries)", facts=dict(VALUES, fc_entries=2), two=True,
   n_entries=99)

# ---- sdc_plan ------------------------------------------------------------------------------------------------------------------------------
# (what sdc_plan_cem and sdc_plan_cem_groups refuse behind their own parameters is the same function: its rules are listed here)
E = "sdc_plan"
SIX_LEFT = dict(t_rel=where(ALL(80), _6=90))
NO_ROWS = "this engine has no feature rows (episodes too long for them): the forecast lives in the feature rows"
ok(E, by="gamma=1.000000")
ok(E, by="gamma=0.500000", obj=1, gamma=0.5, n_cols=8, col=[0, 43, 1, 2, 3, 4, 5, 6], n_steps=T, n_cand=1000000)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "n_cand = 0 must be positive", n_cand=0)
no(E, "n_steps = 0 outside [1, 256]", n_steps=0)
no(E, "n_steps = 257 outside [1, 256]", n_steps=257)
no(E, "null array", actions=0)
no(E, "null array", best=0)
no(E, "null array", share_obs=0)
no(E, "obs / share_obs rows not dword-aligned", obs=GOOD + 2)
ok(E, share_obs=GOOD + 4)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "verify mode checks single steps (sdc_rollout refuses it as well)", facts=dict(debug_flags=1))
ok(E, facts=dict(SIX_LEFT, auto_reset=1), n_steps=5)
no(E, "n_steps = 6 would finish an episode (6 steps left): the auto-reset kills the mark", facts=dict(SIX_LEFT, auto_reset=1), n_steps=6)
no(E, "n_steps = 7 would finish an episode (6 steps left): the auto-reset kills the mark", facts=dict(SIX_LEFT, auto_reset=1), n_steps=7)
ok(E, facts=SIX_LEFT, n_steps=6)
no(E, "n_steps = 7 would run past the end of an episode (6 steps left)", facts=SIX_LEFT, n_steps=7)
no(E, "gamma = 0.000000 outside (0, 1]", obj=1, gamma=0.0)
no(E, "gamma = 1.500000 outside (0, 1]", obj=1, gamma=1.5)
no(E, "n_cols = 9 outside [0, 8]", obj=1, n_cols=9)
no(E, "n_cols = -1 outside [0, 8]", obj=1, n_cols=-1)
no(E, "info column 44 (entry 0) outside [0, 44)", obj=1, n_cols=1, col=[44])
no(E, "info column -1 (entry 1) outside [0, 44)", obj=1, n_cols=2, col=[3, -1])
ok(E, facts=dict(fc_mode=[1, 2, 0, 0]))
no(E, NO_ROWS, facts=dict(fc_mode=[1, 0, 0, 0], has_feat=0))
ok(E, facts=dict(has_feat=0))      # (no forecast set: nothing asked of the feature rows)
no(E, "env 3's feature rows are not valid (a host write to its state since its reset): the forecast lives in the feature rows",
   facts=dict(fc_mode=[0, 0, 2, 0], nofeat=[3, 6]))
no(E, "forecast channel 1 is SDC_FORECAST_VALUES and values is null", facts=dict(VALUES, fc_values=0, fc_entries=9))
ok(E, facts=dict(VALUES, fc_entries=6), n_steps=4)
no(E, "the forecast's values hold 5 entries, 6 are needed (n_steps + 2 at a plan call)", facts=dict(VALUES, fc_entries=5), n_steps=4)
no(E, "n_cand = 0 must be positive", two=True, n_cand=0, n_steps=0)
no(E, "n_steps = 0 outside [1, 256]", two=True, n_steps=0, score=0)
no(E, "null array", two=True, best_action=0, obs=GOOD + 2)
no(E, "obs / share_obs rows not dword-aligned", facts=dict(started=0), two=True, share_obs=GOOD + 1)
no(E, "sdc_reset must be called first", facts=dict(started=0, debug_flags=1), two=True)
no(E, "verify mode checks single steps (sdc_rollout refuses it as well)", facts=dict(debug_flags=1), two=True, n_steps=T + 1)
no(E, "n_steps = 97 would run past the end of an episode (96 steps left)", two=True, n_steps=T + 1, obj=1, gamma=0.0)
no(E, "gamma = 0.000000 outside (0, 1]", facts=dict(VALUES, fc_entries=1), two=True, obj=1, gamma=0.0)
no(E, NO_ROWS, facts=dict(VALUES, fc_entries=1, has_feat=0), two=True)

# ---- sdc_set_plan_terms --------------------------------------------------------------------------------------------------------------------
E = "sdc_set_plan_terms"
INF = float("inf")
LIMIT = dict(n_limits=1, limit_col=[5], limit_side=[1], limit_bound=[2.5], limit_weight=[0.0])
ok(E)
ok(E, terms=0)
ok(E, **LIMIT)
ok(E, n_limits=8, limit_col=[43] * 8, limit_side=[-1] * 8, limit_bound=[-1e9] * 8, limit_weight=[3.0] * 8, n_terminal=8, terminal_col=[0] * 8,
   terminal_weight=[-2.0] * 8)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "n_limits = 9 outside [0, 8]", n_limits=9)
no(E, "n_limits = -1 outside [0, 8]", n_limits=-1)
no(E, "n_terminal = 9 outside [0, 8]", n_terminal=9)
no(E, "n_terminal = -1 outside [0, 8]", n_terminal=-1)
no(E, "limit_col[0] = 44 outside [0, 44)", **dict(LIMIT, limit_col=[44]))
no(E, "limit_side[0] = 0 is neither +1 (upper) nor -1 (lower)", **dict(LIMIT, limit_side=[0]))
no(E, "limit_bound[0] = inf is not finite", **dict(LIMIT, limit_bound=[INF]))
no(E, "limit_weight[0] = inf is not finite", **dict(LIMIT, limit_weight=[INF]))
no(E, "limit_weight[0] = -1.000000 is negative", **dict(LIMIT, limit_weight=[-1.0]))
no(E, "limit_col[1] = -1 outside [0, 44)", n_limits=2, limit_col=[5, -1], limit_side=[1, 1], limit_bound=[0.0, 0.0], limit_weight=[1.0, 1.0])
no(E, "terminal_col[0] = -1 outside [0, 44)", n_terminal=1, terminal_col=[-1], terminal_weight=[1.0])
no(E, "terminal_weight[0] = -inf is not finite", n_terminal=1, terminal_col=[4], terminal_weight=[-INF])
ok(E, n_terminal=1, terminal_col=[4], terminal_weight=[-1.0])
no(E, "n_limits = 9 outside [0, 8]", two=True, n_limits=9, n_terminal=9)
no(E, "limit_side[0] = 2 is neither +1 (upper) nor -1 (lower)", two=True, **dict(LIMIT, limit_side=[2], limit_bound=[INF]))
no(E, "limit_weight[0] = -1.000000 is negative", two=True, n_terminal=1, terminal_col=[44], terminal_weight=[1.0], **dict(LIMIT, limit_weight=[-1.0]))

# ---- sdc_set_critic, sdc_critic_values, sdc_set_plan_critic ------------------------------------------------------------------------------------
# (the parameters: zeros but scale 1, shift 0, flags 0 and what a case plants -- b3 stands for any of the 6459)
E = "sdc_set_critic"
FLAG_BITS = "unknown flag bits (bit 0: feature LayerNorm, bits 1-2: activation)"
ok(E)
ok(E, flags=3)      # (the feature LayerNorm on, relu)
ok(E, flags=2, scale=1e-30, shift=-1e30, b3=-7.5)
no(E, "null handle or params", facts=dict(handle=0), wire=True)
no(E, "null handle or params", p=0)
no(E, "an entry that is not finite", b3=float("nan"))
no(E, "an entry that is not finite", shift=-INF)
no(E, "an entry that is not finite", scale=INF)
no(E, "scale must be positive", scale=0.0)
no(E, "scale must be positive", scale=-2.5)
no(E, FLAG_BITS, flags=8)
no(E, FLAG_BITS, flags=-1)
no(E, "unknown activation code (0 tanh, 1 relu)", flags=4)
no(E, "unknown activation code (0 tanh, 1 relu)", flags=7)
no(E, "an entry that is not finite", two=True, b3=INF, scale=0.0)
no(E, "scale must be positive", two=True, scale=0.0, flags=8)
no(E, FLAG_BITS, two=True, flags=12)      # (and bits 1-2 say 2)
E = "sdc_critic_values"
ok(E, facts=dict(critic=1))
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "sdc_set_critic first")
no(E, "n_rows = 0 must be positive", facts=dict(critic=1), n_rows=0)
no(E, "null array", facts=dict(critic=1), values=0)
no(E, "share_obs / values not dword-aligned", facts=dict(critic=1), share_obs=GOOD + 2)
no(E, "sdc_set_critic first", two=True, n_rows=0)
no(E, "n_rows = -5 must be positive", facts=dict(critic=1), two=True, n_rows=-5, share_obs=0)
no(E, "null array", facts=dict(critic=1), two=True, share_obs=0, values=GOOD + 1)
E = "sdc_set_plan_critic"
ok(E)
ok(E, facts=dict(critic=1), weight=0.5)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "weight = inf is not finite", weight=INF)
no(E, "weight = 0.500000 while no critic is set (sdc_set_critic first)", weight=0.5)
no(E, "weight = -inf is not finite", two=True, weight=-INF)      # (and no critic set)

# ---- sdc_plan_cem --------------------------------------------------------------------------------------------------------------------------
E = "sdc_plan_cem"
ok(E)
ok(E, n_iters=1, iter0=65535)      # (iter0 + n_iters == 65536)
ok(E, n_cand=64, n_elite=64, p_min=1.0 / 3.0, alpha=0.99, fixed=[2, -1, 0])
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "null cem", cem=0)
no(E, "n_iters = 0 must be positive", n_iters=0)
no(E, "iter0 = -1 with n_iters = 1 outside [0, 65536]", iter0=-1)
no(E, "iter0 = 65535 with n_iters = 2 outside [0, 65536]", iter0=65535, n_iters=2)
no(E, "n_cand = 1 outside [2, 64]", n_cand=1)
no(E, "n_cand = 65 outside [2, 64]", n_cand=65)
no(E, "n_elite = 0 outside [1, n_cand = 2]", n_elite=0)
no(E, "n_elite = 3 outside [1, n_cand = 2]", n_elite=3)
ok(E, n_elite=2)
no(E, "fixed_action[1] = 3 outside [-1, 2]", fixed=[-1, 3, -1])
no(E, "fixed_action[0] = -2 outside [-1, 2]", fixed=[-2, 0, 0])
no(E, "alpha = 1.000000 outside [0, 1)", alpha=1.0)
no(E, "alpha = -0.100000 outside [0, 1)", alpha=-0.1)
no(E, "p_min = 0.500000 outside [0, 1/3]", p_min=0.5)
no(E, "p_min = -0.250000 outside [0, 1/3]", p_min=-0.25)
no(E, "n_steps = 0 outside [1, 256]", n_steps=0)
no(E, "null array", cand_score=0)
no(E, "null array", probs=0)
no(E, "obs / share_obs rows not dword-aligned", obs=GOOD + 2)
no(E, "gamma = 0.000000 outside (0, 1]", obj=1, gamma=0.0)
no(E, "null cem", two=True, cem=0, n_steps=0)
no(E, "n_iters = 0 must be positive", two=True, n_iters=0, n_cand=1)
no(E, "n_cand = 1 outside [2, 64]", two=True, n_cand=1, n_elite=0)
no(E, "n_elite = 0 outside [1, n_cand = 2]", two=True, n_elite=0, alpha=1.0)
no(E, "alpha = 1.000000 outside [0, 1)", two=True, alpha=1.0, p_min=0.5)
no(E, "p_min = 0.500000 outside [0, 1/3]", two=True, p_min=0.5, n_steps=0)

# ---- sdc_plan_cem_groups -------------------------------------------------------------------------------------------------------------------
E = "sdc_plan_cem_groups"
FOUR = dict(n_envs=4)      # (the smallest batch that can show a group out of step: two groups of two)


def out_of_step(group, env, first, what):
    return (f"group {group} is out of step: env {env} and its group's first env {first} differ in {what} (the replicas of a group hold one "
            "state: sdc_clone_envs)")


ok(E)
ok(E, facts=FOUR)
ok(E, group_size=8, n_elite=8, group_base=2 ** 31 - 1)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "null cem", cem=0)
no(E, "n_iters = 0 must be positive", n_iters=0)
no(E, "iter0 = 65536 with n_iters = 1 outside [0, 65536]", iter0=65536)
no(E, "group_size = 1 outside [2, 1024]", group_size=1)
no(E, "group_size = 1025 outside [2, 1024]", group_size=1025)
no(E, "n_envs = 8 is not a multiple of group_size = 3", group_size=3)
no(E, "n_envs = 8 is not a multiple of group_size = 16", group_size=16)
no(E, "n_elite = 3 outside [1, group_size = 2]", n_elite=3)
no(E, "n_elite = 0 outside [1, group_size = 2]", n_elite=0)
no(E, "group_base = -1 is negative", group_base=-1)
no(E, "fixed_action[2] = 3 outside [-1, 2]", fixed=[0, 0, 3])
no(E, "alpha = 1.000000 outside [0, 1)", alpha=1.0)
no(E, "p_min = 0.500000 outside [0, 1/3]", p_min=0.5)
no(E, "n_steps = 257 outside [1, 256]", n_steps=257)
no(E, "null array", step_actions=0)
no(E, "null array", best_seq=0)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, out_of_step(1, 3, 2, "episode step"), facts=dict(FOUR, t_rel=[0, 0, 0, 1]))
no(E, out_of_step(0, 1, 0, "data-centre config"), facts=dict(FOUR, n_cfg=2, cfg_ids=[0, 1, 0, 0]))
no(E, out_of_step(1, 3, 2, "location"), facts=dict(FOUR, n_loc=2, loc_ids=[1, 1, 0, 1]))
no(E, out_of_step(0, 1, 0, "feature-row flag"), facts=dict(FOUR, nofeat=[1]))
ok(E, facts=dict(FOUR, n_cfg=2, n_loc=2, t_rel=[3, 3, 0, 0], cfg_ids=[1, 1, 0, 0], loc_ids=[0, 0, 1, 1], nofeat=[2, 3]))      # (groups may differ)
no(E, "n_envs = 8 is not a multiple of group_size = 3", two=True, group_size=3, alpha=1.0)
no(E, "n_iters = 0 must be positive", two=True, n_iters=0, group_size=1)
no(E, "n_elite = 5 outside [1, group_size = 4]", two=True, group_size=4, n_elite=5, group_base=-1)
no(E, "group_base = -1 is negative", two=True, group_base=-1, p_min=0.5)
no(E, "p_min = 0.500000 outside [0, 1/3]", two=True, p_min=0.5, cand=0)
no(E, out_of_step(1, 3, 2, "episode step"), facts=dict(FOUR, t_rel=[0, 0, 0, 1], cfg_ids=[0, 0, 0, 1], n_cfg=2), two=True)
# (behind sdc_plan's rules, the forecast's among them: a forecast that is too short is named before a group out of step)
no(E, "the forecast's values hold 2 entries, 3 are needed (n_steps + 2 at a plan call)", facts=dict(FOUR, t_rel=[0, 0, 0, 1], fc_entries=2, **VALUES),
   two=True)

# ---- sdc_rollout_stats ---------------------------------------------------------------------------------------------------------------------
# (what the four statistics calls refuse alike about their arrays and the engine is one function: its rules are listed here)
E = "sdc_rollout_stats"
NULL_STATS = "null array (stats, returns, counts, obs and share_obs are required)"
ROWS_DWORD = "counts / obs / share_obs / rew / info / final_obs rows not dword-aligned"
ok(E)
ok(E, n_steps=T, accumulate=1, rew=0, done=0, info=0, final_obs=0)      # (the single-step arrays are optional)
ok(E, facts=dict(all_policies=1), actions=0)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "n_steps = 0 must be positive", n_steps=0)
no(E, NULL_STATS, stats=0)
no(E, NULL_STATS, counts=0)
no(E, NULL_STATS, share_obs=0)
ok(E, stats=GOOD + 16, returns=GOOD + 32)
no(E, "stats / returns not 16-byte aligned", returns=GOOD + 8)
no(E, "stats / returns not 16-byte aligned", stats=GOOD + 4)
no(E, ROWS_DWORD, counts=GOOD + 2)
no(E, ROWS_DWORD, final_obs=GOOD + 1)
ok(E, info=GOOD + 4)
no(E, "accumulate = 2 outside {0, 1}", accumulate=2)
no(E, "accumulate = -1 outside {0, 1}", accumulate=-1)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "verify mode checks single steps (sdc_rollout refuses it as well)", facts=dict(debug_flags=1))
no(E, "actions may only be NULL when every agent slot has a policy", actions=0)
no(E, "n_steps = 97 would run past the end of an episode (96 steps left)", n_steps=T + 1)
no(E, "n_steps = 0 must be positive", two=True, n_steps=0, stats=0)
no(E, NULL_STATS, two=True, returns=0, stats=GOOD + 8)
no(E, "stats / returns not 16-byte aligned", two=True, stats=GOOD + 8, obs=GOOD + 2)
no(E, ROWS_DWORD, two=True, obs=GOOD + 2, accumulate=2)
no(E, "accumulate = 2 outside {0, 1}", facts=dict(started=0), two=True, accumulate=2)
no(E, "sdc_reset must be called first", facts=dict(started=0, debug_flags=1), two=True)
no(E, "verify mode checks single steps (sdc_rollout refuses it as well)", facts=dict(debug_flags=1), two=True, actions=0)
no(E, "actions may only be NULL when every agent slot has a policy", two=True, actions=0, n_steps=T + 1)

# ---- sdc_rollout_actor_stats ---------------------------------------------------------------------------------------------------------------
E = "sdc_rollout_actor_stats"
ok(E, facts=ACT)
ok(E, facts=ACT, n_steps=T, sample=1, policy_counts=GOOD + 4, policy_sums=GOOD + 16)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "n_steps = 0 must be positive", facts=ACT, n_steps=0)
no(E, NULL_STATS, facts=ACT, obs=0)
no(E, "sdc_reset must be called first", facts=dict(ACT, started=0))
no(E, "verify mode checks single steps (sdc_rollout refuses it as well)", facts=dict(ACT, debug_flags=1))
no(E, "sample = 2 outside {0, 1}", facts=ACT, sample=2)
no(E, "policy_counts and policy_sums are given together or not at all", facts=ACT, policy_counts=GOOD)
no(E, "policy_counts and policy_sums are given together or not at all", facts=ACT, policy_sums=GOOD)
no(E, "policy_sums not 16-byte aligned", facts=ACT, policy_counts=GOOD, policy_sums=GOOD + 8)
no(E, "policy_counts not dword-aligned", facts=ACT, policy_counts=GOOD + 2, policy_sums=GOOD)
no(E, "sdc_set_actor all three agents first")
no(E, ONE_ACTIVATION, facts=dict(ACT, actor_act=[1, 0, 1]))
no(E, NO_OBS, facts=dict(ACT, latch=0))
no(E, COMMON_CASE, facts=dict(ACT, racks=33))
ok(E, facts=dict(ACT, racks=32))
no(E, "n_steps = 97 would run past the end of an episode (96 steps left)", facts=ACT, n_steps=T + 1)
no(E, "accumulate = 3 outside {0, 1}", two=True, accumulate=3, sample=2)
no(E, "sample = 2 outside {0, 1}", two=True, sample=2)      # (and no actor set)
no(E, "policy_counts and policy_sums are given together or not at all", two=True, policy_sums=GOOD + 8)
no(E, "policy_sums not 16-byte aligned", two=True, policy_counts=GOOD + 2, policy_sums=GOOD + 8)
no(E, "sdc_set_actor all three agents first", two=True, n_steps=T + 1)
no(E, NO_OBS, facts=dict(ACT, latch=0, racks=40), two=True)
no(E, COMMON_CASE, facts=dict(ACT, racks=40), two=True, n_steps=T + 1)

# ---- sdc_rollout_cem_stats -----------------------------------------------------------------------------------------------------------------
E = "sdc_rollout_cem_stats"
NULL_PLAN = "null array (probs, best_seq, best_score, best_action, cand and cand_score are required)"
PLAN_STATS = dict(plan_counts=GOOD, plan_sums=GOOD)
ok(E, by="k_max=1")
ok(E, by="k_max=4", horizon=4, resume=1, resume_steps=4, warm_start=1, n_steps=T, idle=[2, 2, 2], **PLAN_STATS)      # (resume_steps == horizon)
ok(E, facts=dict(auto_reset=1, t_rel=ALL(T - 3)), by="k_max=2", horizon=8, n_steps=3)      # (the auto-reset: the plan stops a step short)
ok(E, facts=dict(t_rel=ALL(T - 1), fc_mode=[3, 3, 3, 3]), by="k_max=0")      # (every decision idles: the forecast is not asked)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "n_steps = 0 must be positive", n_steps=0)
no(E, NULL_STATS, returns=0)
no(E, "stats / returns not 16-byte aligned", returns=GOOD + 8)
no(E, ROWS_DWORD, counts=GOOD + 2)
no(E, "accumulate = 2 outside {0, 1}", accumulate=2)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "verify mode checks single steps (sdc_rollout refuses it as well)", facts=dict(debug_flags=1))
no(E, "null mpc", mpc=0)
no(E, "horizon = 0 outside [1, 256]", horizon=0)
no(E, "horizon = 257 outside [1, 256]", horizon=257)
no(E, "warm_start = 2 outside {0, 1}", warm_start=2)
no(E, "resume = -1 outside {0, 1}", resume=-1)
no(E, "resume_steps = 0 outside [1, horizon = 1]", resume=1, resume_steps=0)
no(E, "resume_steps = 5 outside [1, horizon = 4]", horizon=4, resume=1, resume_steps=5)
ok(E, by="k_max=4", horizon=4, resume_steps=99)      # (read only while resuming)
no(E, "idle_action[2] = 3 outside [0, 2]", idle=[1, 1, 3])
no(E, "idle_action[0] = -1 outside [0, 2]", idle=[-1, 1, 2])
no(E, "n_iters = 0 must be positive", n_iters=0)
no(E, "iter0 = 65535 with n_iters = 2 outside [0, 65536]", iter0=65535, n_iters=2)
no(E, "n_cand = 65 outside [2, 64]", n_cand=65)
no(E, "n_elite = 3 outside [1, n_cand = 2]", n_elite=3)
no(E, "fixed_action[1] = 3 outside [-1, 2]", fixed=[-1, 3, -1])
no(E, "alpha = 1.000000 outside [0, 1)", alpha=1.0)
no(E, "p_min = 0.500000 outside [0, 1/3]", p_min=0.5)
for nm in ("probs", "best_seq", "best_score", "best_action", "cand", "cand_score"):
    no(E, NULL_PLAN, **{nm: 0})
no(E, "probs / best_score / cand_score not 8-byte aligned", probs=GOOD + 4)
no(E, "probs / best_score / cand_score not 8-byte aligned", cand_score=GOOD + 4)
no(E, "best_seq / best_action / cand not dword-aligned", best_seq=GOOD + 2)
no(E, "plan_counts and plan_sums are given together or not at all", plan_sums=GOOD)
no(E, "plan_counts and plan_sums are given together or not at all", plan_counts=GOOD)
no(E, "plan_sums not 16-byte aligned", plan_counts=GOOD, plan_sums=GOOD + 8)
no(E, "plan_counts not dword-aligned", plan_counts=GOOD + 2, plan_sums=GOOD)
no(E, "gamma = 0.000000 outside (0, 1]", obj=1, gamma=0.0)
no(E, "gamma = 1.500000 outside (0, 1]", obj=1, gamma=1.5)
no(E, "n_cols = 9 outside [0, 8]", obj=1, n_cols=9)
no(E, "info column 44 (entry 0) outside [0, 44)", obj=1, n_cols=1, col=[44])
no(E, "n_steps = 97 would run past the end of an episode (96 steps left)", n_steps=T + 1)
ok(E, facts=dict(VALUES, fc_entries=6), by="k_max=4", horizon=4, n_steps=9)
no(E, "the forecast's values hold 5 entries, 6 are needed (n_steps + 2 at a plan call)", facts=dict(VALUES, fc_entries=5), horizon=4, n_steps=9)
no(E, NO_ROWS, facts=dict(fc_mode=[0, 0, 0, 1], has_feat=0))
# the order of the refusals, as tests/test_gpu_mpc_stats.py pins it, and on
no(E, "n_steps = 0 must be positive", two=True, n_steps=0, mpc=0)
no(E, "horizon = 0 outside [1, 256]", two=True, horizon=0, n_iters=0)
no(E, "n_iters = 0 must be positive", two=True, n_iters=0, probs=0)
no(E, NULL_PLAN, two=True, probs=0, plan_counts=GOOD, plan_sums=GOOD + 8)
no(E, "plan_sums not 16-byte aligned", two=True, plan_counts=GOOD, plan_sums=GOOD + 8, obj=1, gamma=0.0)
no(E, "gamma = 0.000000 outside (0, 1]", two=True, obj=1, gamma=0.0, n_steps=T + 1)
no(E, "verify mode checks single steps (sdc_rollout refuses it as well)", facts=dict(debug_flags=1), two=True, mpc=0)
no(E, "probs / best_score / cand_score not 8-byte aligned", two=True, best_score=GOOD + 4, cand=GOOD + 2)
no(E, "best_seq / best_action / cand not dword-aligned", two=True, cand=GOOD + 2, plan_counts=GOOD)
no(E, "n_steps = 97 would run past the end of an episode (96 steps left)", facts=dict(VALUES, fc_entries=1), two=True, n_steps=T + 1)

# ---- sdc_rollout_cem_groups_stats ----------------------------------------------------------------------------------------------------------
E = "sdc_rollout_cem_groups_stats"
NULL_GROUP_PLAN = "null array (probs, best_seq, best_score, best_action, step_actions, cand and cand_score are required)"
GROUP_STATS = dict(plan_counts=GOOD, plan_sums=GOOD, diverged=GOOD)
TOGETHER = "plan_counts, plan_sums and diverged are given together or not at all"
ok(E, by="k_max=1")
ok(E, by="k_max=1", sync_first=1, **GROUP_STATS)
ok(E, facts=FOUR, by="k_max=3", horizon=3, n_steps=T)
ok(E, facts=dict(t_rel=ALL(T - 1), fc_mode=[3, 3, 3, 3]), by="k_max=0")      # (every decision idles: the forecast is not asked)
no(E, "null handle", facts=dict(handle=0), wire=True)
no(E, "n_steps = 0 must be positive", n_steps=0)
no(E, NULL_STATS, obs=0)
no(E, "sdc_reset must be called first", facts=dict(started=0))
no(E, "null mpc", mpc=0)
no(E, "horizon = 257 outside [1, 256]", horizon=257)
no(E, "warm_start = -1 outside {0, 1}", warm_start=-1)
no(E, "resume = 2 outside {0, 1}", resume=2)
no(E, "resume_steps = 2 outside [1, horizon = 1]", resume=1, resume_steps=2)
no(E, "idle_action[1] = 3 outside [0, 2]", idle=[0, 3, 0])
no(E, "sync_first = 2 outside {0, 1}", sync_first=2)
no(E, "sync_first = -1 outside {0, 1}", sync_first=-1)
no(E, "sync_first with resume (behind the sync the first planned decision starts fresh: nothing can be resumed)", sync_first=1, resume=1, resume_steps=1)
no(E, "n_iters = 0 must be positive", n_iters=0)
no(E, "group_size = 1 outside [2, 1024]", group_size=1)
no(E, "n_envs = 8 is not a multiple of group_size = 3", group_size=3)
no(E, "n_elite = 3 outside [1, group_size = 2]", n_elite=3)
no(E, "group_base = -1 is negative", group_base=-1)
no(E, "alpha = 1.000000 outside [0, 1)", alpha=1.0)
for nm in ("probs", "best_seq", "best_score", "best_action", "step_actions", "cand", "cand_score"):
    no(E, NULL_GROUP_PLAN, **{nm: 0})
no(E, "probs / best_score / cand_score not 8-byte aligned", best_score=GOOD + 4)
no(E, "best_seq / best_action / step_actions / cand not dword-aligned", step_actions=GOOD + 2)
for some in (("plan_counts",), ("plan_sums",), ("diverged",), ("plan_counts", "plan_sums"), ("plan_sums", "diverged"), ("plan_counts", "diverged")):
    no(E, TOGETHER, **{nm: GOOD for nm in some})
no(E, "plan_sums not 16-byte aligned", **dict(GROUP_STATS, plan_sums=GOOD + 8))
no(E, "plan_counts / diverged not dword-aligned", **dict(GROUP_STATS, plan_counts=GOOD + 2))
no(E, "plan_counts / diverged not dword-aligned", **dict(GROUP_STATS, diverged=GOOD + 2))
no(E, "gamma = 0.000000 outside (0, 1]", obj=1, gamma=0.0)
no(E, "n_steps = 97 would run past the end of an episode (96 steps left)", n_steps=T + 1)
# a replica ahead of its group's first env: without a sync the episode ends where the replica's does, and the group is out of step;
# with one, every replica stands where its group's first env stands
AHEAD = dict(FOUR, t_rel=[0, 90, 0, 0])
no(E, "n_steps = 7 would run past the end of an episode (6 steps left)", facts=AHEAD, n_steps=7)
no(E, out_of_step(0, 1, 0, "episode step"), facts=AHEAD, n_steps=6)
ok(E, facts=AHEAD, by="k_max=1", n_steps=T, sync_first=1)
no(E, "n_steps = 97 would run past the end of an episode (96 steps left)", facts=AHEAD, n_steps=T + 1, sync_first=1)
no(E, "n_steps = 7 would run past the end of an episode (6 steps left)", facts=dict(FOUR, t_rel=[0, 0, 90, 0]), n_steps=7, sync_first=1)
no(E, out_of_step(0, 1, 0, "data-centre config"), facts=dict(FOUR, n_cfg=2, cfg_ids=[0, 1, 0, 0]))
no(E, out_of_step(1, 3, 2, "location"), facts=dict(FOUR, n_loc=2, loc_ids=[0, 0, 0, 1]))
no(E, out_of_step(1, 3, 2, "feature-row flag"), facts=dict(FOUR, nofeat=[3]))
ok(E, facts=dict(VALUES, fc_entries=3), by="k_max=1")
no(E, "the forecast's values hold 2 entries, 3 are needed (n_steps + 2 at a plan call)", facts=dict(VALUES, fc_entries=2))
# the order of the refusals, as tests/test_gpu_mpc_groups.py pins it, and on
no(E, "n_steps = 0 must be positive", two=True, n_steps=0, mpc=0)
no(E, "horizon = 0 outside [1, 256]", two=True, horizon=0, n_iters=0)
no(E, "n_iters = 0 must be positive", two=True, n_iters=0, probs=0)
no(E, NULL_GROUP_PLAN, two=True, probs=0, **dict(GROUP_STATS, plan_sums=GOOD + 8))
no(E, "plan_sums not 16-byte aligned", two=True, obj=1, gamma=0.0, **dict(GROUP_STATS, plan_sums=GOOD + 8))
no(E, "gamma = 0.000000 outside (0, 1]", two=True, obj=1, gamma=0.0, n_steps=T + 1)
no(E, "sync_first = 2 outside {0, 1}", two=True, sync_first=2, n_iters=0)
no(E, "n_envs = 8 is not a multiple of group_size = 3", two=True, group_size=3, alpha=1.0)
no(E, out_of_step(1, 3, 2, "episode step"), facts=dict(FOUR, t_rel=[0, 0, 0, 1], fc_entries=2, **VALUES), two=True)
no(E, "idle_action[0] = 3 outside [0, 2]", two=True, idle=[3, 0, 0], sync_first=2)
no(E, "sync_first with resume (behind the sync the first planned decision starts fresh: nothing can be resumed)", two=True, sync_first=1, resume=1,
   resume_steps=1, group_size=1)
