"""SdcEngine: N SustainDC environment instances resident on one MI355X, driven through the C-ABI.

PyTorch is plumbing here: it owns the obs / action / reward / info device buffers and the HIP stream;
every call lands in the hand-written kernels of csrc/ (which step kernel a call launches: csrc/sdc_dispatch.hpp; sdc_reset_kernel at
episode boundaries).  How the methods below share their plumbing -- `_args.py`'s validators, `_call`, `_p` --: DESIGN.md 4.18.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _args as A
from . import _lib as L
from ._args import group_sync_pairs       # noqa: F401  (vec_env imports it from here)

_STATE_DTYPES = A.STATE_SCALARS     # (an env's scalar states: tests iterate over the names)
# a full checkpoint: the raw records + every array the kernels own
# "hist" first: injecting the ring drops the order-statistic trackers, which "header" then restores
_CHECKPOINT = ["hist", "record", "header", "qwin", "t_win", "wb_win", "qtab"]
# what a checkpoint's arrays only make sense with: a load into an engine that differs in any of these is refused
_META_MUST_MATCH = ("layout", "n_envs", "episode_steps", "hist_cap", "queue_max_len", "max_roll_days", "n_locations",
                    "n_dc_configs", "env_index_base")
# ... and a snapshot's rows: the same, but they may go to an engine of another size, and to any slot of it
_SNAPSHOT_MUST_MATCH = tuple(k for k in _META_MUST_MATCH if k not in ("n_envs", "env_index_base"))


class EnvSnapshot:
    """Env states in a device buffer (SdcEngine.snapshot): `rows` uint8 [n, row_bytes] -- row k is env `envs[k]`'s complete state in
    the library's engine-independent layout (include/sustaindc_hip.h sdc_snapshot_envs) --, `manifest` int32 [n, SNAPSHOT_MANIFEST]
    (host: what the library checks a restore against), `meta` (the state layout and the configuration the rows only make sense with)
    and `envs`, the source env ids.  `extra`: host-side per-row entries a wrapper keeps with the rows (SustainDCVecEnv)."""

    def __init__(self, rows, manifest, meta, envs, extra=None):
        self.rows, self.manifest, self.meta, self.envs = rows, manifest, meta, envs
        self.extra = extra if extra is not None else {}

    def __len__(self):
        return int(self.envs.shape[0])

    @property
    def nbytes(self) -> int:
        return int(self.rows.numel())

    def to(self, device):
        """The same snapshot with its rows on another device (restore into an engine on another GPU)."""
        return EnvSnapshot(self.rows.to(device), self.manifest, self.meta, self.envs, self.extra)


class EnvMark:
    """What the next `max_steps` steps can change in envs (SdcEngine.mark): `rows` uint8 [n, row_bytes] on the engine's device -- row k
    belongs to env `envs[k]` (include/sustaindc_hip.h sdc_mark_envs: ~2.3 KB per env for 16 steps, against a snapshot's ~146 KB) --,
    `manifest` int32 [n, MARK_MANIFEST] (host: what the library checks a rewind against) and `envs`.  A mark goes back into the engine
    and the envs it was taken from, and only while it is the envs' latest mark and they have not been reset, written or overwritten."""

    def __init__(self, rows, manifest, envs, max_steps, whole):
        self.rows, self.manifest, self.envs, self.max_steps, self.whole = rows, manifest, envs, int(max_steps), bool(whole)
        self._pos = None

    def __len__(self):
        return int(self.envs.shape[0])

    @property
    def nbytes(self) -> int:
        return int(self.rows.numel())

    def positions(self, envs):
        """the rows of `envs` (an int32 array); ValueError for an env the mark does not hold"""
        if self._pos is None:
            self._pos = {int(e): k for k, e in enumerate(self.envs.tolist())}
        try:
            return np.asarray([self._pos[int(e)] for e in envs.tolist()], dtype=np.int64)
        except KeyError as ex:
            raise ValueError(f"rewind: env {ex.args[0]} is not one of the mark's envs") from None


class PlanResult:
    """What SdcEngine.plan returns, all on the engine's device: `best` int32 [N] the winning candidate of every env, `action` int32
    [N, 3] its first action (SustainDCVecEnv.plan: the agent subset's columns), `score` float64 [M, N] and `returns` float64 [M, N, 3]
    (the three agents' discounted returns of every candidate)."""

    def __init__(self, best, action, score, returns):
        self.best, self.action, self.score, self.returns = best, action, score, returns


class CEMResult:
    """What SdcEngine.plan_cem returns, all on the engine's device: `action` int32 [N, 3] the first action of every env's best sequence
    (SustainDCVecEnv.plan_cem: the agent subset's columns), `best_seq` int32 [K, N, 3] that sequence, `best_score` float64 [I, N] its
    score after each iteration, `probs` float64 [K, N, 3, 3] the refitted distributions, `cand` int32 [M, K, N, 3] and `cand_score`
    float64 [M, N] the last iteration's candidates and their scores."""

    def __init__(self, action, best_seq, best_score, probs, cand, cand_score):
        self.action, self.best_seq, self.best_score, self.probs, self.cand, self.cand_score = action, best_seq, best_score, probs, cand, cand_score


class GroupCEMResult:
    """What SdcEngine.plan_cem_groups returns, all on the engine's device; G = N / group_size groups: `action` int32 [G, 3] the first
    action of every group's best sequence (SustainDCVecEnv.plan_cem_groups: the agent subset's columns), `step_actions` int32 [N, 3]
    (the vec env: [N, n_agents]) the same broadcast to every replica -- what to step with so that a group stays identical --,
    `best_seq` int32 [K, G, 3] that sequence, `best_score` float64 [I, G] its score after each iteration, `probs` float64
    [K, G, 3, 3] the refitted distributions, `cand` int32 [K, N, 3] and `cand_score` float64 [N] the last iteration's sequences
    (replica r of group g played cand[:, g R + r]) and their scores."""

    def __init__(self, action, step_actions, best_seq, best_score, probs, cand, cand_score):
        self.action, self.step_actions, self.best_seq, self.best_score = action, step_actions, best_seq, best_score
        self.probs, self.cand, self.cand_score = probs, cand, cand_score


# EpisodeStats.summary: the reference logger's quantities (harl/envs/sustaindc/sustaindc_logger.py), name -> (info column, kind)
_SUMMARY = {
    "average_net_energy": ("bat_total_energy_with_battery_KWh", "mean"),      # sustaindc_logger.py:87, :131
    "average_ite_power": ("dc_ITE_total_power_kW", "mean"),                   # :93, :132
    "average_ct_power": ("dc_CT_total_power_kW", "mean"),                     # :94, :133
    "average_chiller_power": ("dc_Compressor_total_power_kW", "mean"),        # :95, :134
    "average_hvac_power": ("dc_HVAC_total_power_kW", "mean"),                 # :96, :135
    "average_CO2_footprint": ("bat_CO2_footprint", "mean"),                   # :88, :137
    "total_water_usage": ("dc_water_usage", "total"),                         # :89, :138
    "total_tasks_in_queue": ("ls_tasks_in_queue", "total"),                   # :91, :140
    "total_tasks_dropped": ("ls_tasks_dropped", "total"),                     # :92, :141
    "average_hvac_power_on_use": ("dc_HVAC_total_power_kW", "positive"),      # :98-99, :153
}


class EpisodeStats:
    """What SdcEngine.rollout_stats / evaluate return: per-env statistics of the steps taken, on the engine's device (sdc_rollout_stats,
    include/sustaindc_hip.h).  `stats` float64 [4, N, 44] -- `sum`, `min`, `max`, `n_pos` (the number of steps with a positive value) are
    its [N, 44] views, one row per env and one column per info key (dc_rl_amd._lib.INFO_COLS) --, `returns` float64 [N, 3] the three
    agents' summed rewards, `counts` int32 [N, 2] with the views `steps` [N] (steps reduced) and `fault` [N] (the OR of the steps'
    info[fault] bits).  `policy`: the PolicyStats of the same steps from `rollout_actor_stats` / `evaluate(actors=True)`, None from
    `rollout_stats`.  `plan`: the PlanStats of the same steps from `rollout_cem_stats` / `evaluate(mpc=)`, None from the others; `mpc`:
    the MPCCarry `rollout_cem_stats` leaves (what a later call resumes from), None from the others.  From `evaluate` every tensor has a
    leading [E] dimension, one entry per episode."""

    def __init__(self, stats, returns, counts, policy=None, *, plan=None):
        self.stats, self.returns, self.counts, self.policy, self.plan = stats, returns, counts, policy, plan
        self.mpc = None

    sum = property(lambda self: self.stats.select(-3, 0))
    min = property(lambda self: self.stats.select(-3, 1))
    max = property(lambda self: self.stats.select(-3, 2))
    n_pos = property(lambda self: self.stats.select(-3, 3))
    steps = property(lambda self: self.counts[..., 0])
    fault = property(lambda self: self.counts[..., 1])

    def col(self, name: str, field: str = "sum"):
        """The [N] column of `field` ("sum", "min", "max", "n_pos") for the reference's info key `name`; ValueError for an unknown one."""
        if name not in L.INFO_IDX:
            raise ValueError(f"col: {name!r} is not an info column (dc_rl_amd._lib.INFO_COLS)")
        if field not in ("sum", "min", "max", "n_pos"):
            raise ValueError(f"col: field {field!r} is not one of sum, min, max, n_pos")
        return getattr(self, field)[..., L.INFO_IDX[name]]

    def summary(self) -> dict:
        """The reference logger's episode quantities (harl/envs/sustaindc/sustaindc_logger.py:126-149) on the host, fp64:
        {"per_env": {name: array [N] (or [E, N])}, "batch": {name: float (or array [E])}, "steps": ..., "fault": ...}.  Per env the
        logger's formulas with the env's own sums and step count; over the batch with the sums over the envs and the sum of their step
        counts, which is what the logger accumulates (:86-101: one `step_count` per env and step).
          average_net_energy, average_ite_power, average_ct_power, average_chiller_power, average_hvac_power, average_CO2_footprint
              = sum / steps (:131-137);   total_water_usage, total_tasks_in_queue, total_tasks_dropped = sum (:138-141);
          average_hvac_power_on_use = sum / n_pos of dc_HVAC_total_power_kW: the mean over the steps where it was positive (:98-99,
              :153; the power is never negative, so the other steps add nothing to the sum); NaN where it never was.
        A quantity of an env that took no step is 0, as in the logger (:142-150)."""
        s, n = self.sum.cpu().numpy(), self.n_pos.cpu().numpy()
        steps = self.steps.cpu().numpy().astype(np.float64)
        tot_steps = steps.sum(axis=-1)
        per_env, batch = {}, {}
        with np.errstate(divide="ignore", invalid="ignore"):
            for name, (key, kind) in _SUMMARY.items():
                c = L.INFO_IDX[key]
                x, bx = s[..., c], s[..., c].sum(axis=-1)
                if kind == "mean":
                    per_env[name] = np.where(steps > 0, x / steps, 0.0)
                    batch[name] = np.where(tot_steps > 0, bx / tot_steps, 0.0)
                elif kind == "total":
                    per_env[name], batch[name] = x, bx
                else:
                    per_env[name], batch[name] = x / n[..., c], bx / n[..., c].sum(axis=-1)
        batch = {k: (float(v) if np.ndim(v) == 0 else np.asarray(v)) for k, v in batch.items()}
        return {"per_env": per_env, "batch": batch, "steps": self.steps.cpu().numpy(), "fault": self.fault.cpu().numpy()}


class PolicyStats:
    """What the three actors did over the steps of an EpisodeStats (sdc_rollout_actor_stats, include/sustaindc_hip.h), per env and agent
    (ls, dc, bat), on the engine's device: `counts` int32 [N, 3, 5] with the views `action_counts` [N, 3, 3] (steps on which action
    0 / 1 / 2 was played), `switches` [N, 3] (steps whose action differs from the step before) and `last_action` [N, 3] (-1: no step
    yet); `sums` float64 [N, 3, 2] with the views `logp` (the summed log-probability of the actions played) and `entropy` (the summed
    entropy of the distributions they were chosen from).  From `evaluate` every tensor has a leading [E] dimension."""

    def __init__(self, counts, sums):
        self.counts, self.sums = counts, sums

    action_counts = property(lambda self: self.counts[..., :3])
    switches = property(lambda self: self.counts[..., L.POLICY_SWITCHES])
    last_action = property(lambda self: self.counts[..., L.POLICY_LAST])
    logp = property(lambda self: self.sums[..., L.POLICY_LOGP])
    entropy = property(lambda self: self.sums[..., L.POLICY_ENTROPY])

    def summary(self) -> dict:
        """Per-step quantities on the host, fp64: {"per_env": {name: array [N, 3] (or [E, N, 3])}, "batch": {name: array [3] (or
        [E, 3])}, "steps": array [N, 3]}, the last axis the agents (ls, dc, bat).  With steps = the three action counts' sum:
          action_frequency  [..., 3 agents, 3 actions] = action_counts / steps;
          mean_entropy = entropy / steps;   mean_logp = logp / steps;
          switch_rate = switches / max(steps - 1, 1): the share of step-to-step transitions on which the agent changed its action.
        Over the batch the same formulas with the sums over the envs (the transitions: the sum of the envs' max(steps - 1, 1)).  A
        quantity of an (env, agent) that took no step is 0."""
        n = self.action_counts.cpu().numpy().astype(np.float64)
        sw = self.switches.cpu().numpy().astype(np.float64)
        lp, ent = self.logp.cpu().numpy(), self.entropy.cpu().numpy()
        steps = n.sum(axis=-1)
        trans = np.maximum(steps - 1.0, 1.0)
        per_env, batch = {}, {}
        with np.errstate(divide="ignore", invalid="ignore"):
            def ratio(x, d):
                return np.where(d > 0, x / d, 0.0)
            bsteps = steps.sum(axis=-2)
            per_env["action_frequency"] = ratio(n, steps[..., None])
            batch["action_frequency"] = ratio(n.sum(axis=-3), bsteps[..., None])
            for name, x in (("mean_entropy", ent), ("mean_logp", lp)):
                per_env[name], batch[name] = ratio(x, steps), ratio(x.sum(axis=-2), bsteps)
            per_env["switch_rate"], batch["switch_rate"] = sw / trans, sw.sum(axis=-2) / trans.sum(axis=-2)
        return {"per_env": per_env, "batch": batch, "steps": steps.astype(np.int64)}


class PlanStats:
    """What the planner did over the steps of an EpisodeStats (sdc_rollout_cem_stats, include/sustaindc_hip.h), on the engine's device:
    `counts` int32 [N, 3, 5] per env and agent (ls, dc, bat) with the views `action_counts` [N, 3, 3] (steps on which action 0 / 1 / 2
    was played, idle decisions included), `switches` [N, 3] (steps whose action differs from the step before) and `last_action` [N, 3]
    (-1: no step yet); `sums` float64 [N, 4] per env with the views `score` (the summed score the planner predicted for the sequence
    it chose, over the planned decisions), `gain` (the summed improvement of that score over the CEM iterations: last minus first),
    `planned` and `idle` (the number of decisions of either kind, as doubles).  From `evaluate` every tensor has a leading [E]
    dimension.  From `rollout_cem_groups_stats` (sdc_rollout_cem_groups_stats) the leading dimension N is the number of groups G, and
    `diverged` is an int32 [G] tensor: per group the number of (step, replica) pairs at which a replica's rew, done or info row (without
    info[reserved]) differed from its group's first env's in any bit -- 0 while the group holds one state; None from the per-env call."""

    def __init__(self, counts, sums, diverged=None):
        self.counts, self.sums, self.diverged = counts, sums, diverged

    action_counts = property(lambda self: self.counts[..., :3])
    switches = property(lambda self: self.counts[..., L.POLICY_SWITCHES])
    last_action = property(lambda self: self.counts[..., L.POLICY_LAST])
    score = property(lambda self: self.sums[..., L.PLAN_SCORE])
    gain = property(lambda self: self.sums[..., L.PLAN_GAIN])
    planned = property(lambda self: self.sums[..., L.PLAN_PLANNED])
    idle = property(lambda self: self.sums[..., L.PLAN_IDLE])

    def summary(self) -> dict:
        """Per-decision quantities on the host, fp64: {"per_env": {...}, "batch": {...}, "steps": array [N, 3] (or [E, N, 3]),
        "planned": array [N], "idle": array [N]}.  With steps = the three action counts' sum, per env and agent (last axis: ls, dc, bat):
          action_frequency  [..., 3 agents, 3 actions] = action_counts / steps;
          switch_rate = switches / max(steps - 1, 1);
        and per env:  mean_score = score / planned;   mean_gain = gain / planned -- per planned decision.
        Over the batch the same formulas with the sums over the envs (the transitions: the sum of the envs' max(steps - 1, 1)).  A
        quantity of an env that took no step, or planned no decision, is 0, never NaN.  With `diverged` (replica groups: read "env" as
        "group") the dict also carries "diverged": array [G] (or [E, G])."""
        n = self.action_counts.cpu().numpy().astype(np.float64)
        sw = self.switches.cpu().numpy().astype(np.float64)
        score, gain = self.score.cpu().numpy(), self.gain.cpu().numpy()
        planned, idle = self.planned.cpu().numpy(), self.idle.cpu().numpy()
        steps = n.sum(axis=-1)
        trans = np.maximum(steps - 1.0, 1.0)
        per_env, batch = {}, {}
        with np.errstate(divide="ignore", invalid="ignore"):
            def ratio(x, d):
                return np.where(d > 0, x / d, 0.0)
            bsteps, bplanned = steps.sum(axis=-2), planned.sum(axis=-1)
            per_env["action_frequency"] = ratio(n, steps[..., None])
            batch["action_frequency"] = ratio(n.sum(axis=-3), bsteps[..., None])
            per_env["switch_rate"], batch["switch_rate"] = sw / trans, sw.sum(axis=-2) / trans.sum(axis=-2)
            for name, x in (("mean_score", score), ("mean_gain", gain)):
                per_env[name], batch[name] = ratio(x, planned), ratio(x.sum(axis=-1), bplanned)
        batch = {k: (float(v) if np.ndim(v) == 0 else np.asarray(v)) for k, v in batch.items()}
        out = {"per_env": per_env, "batch": batch, "steps": steps.astype(np.int64), "planned": planned.astype(np.int64),
               "idle": idle.astype(np.int64)}
        if self.diverged is not None:
            out["diverged"] = self.diverged.cpu().numpy().astype(np.int64)
        return out


class GAEResult:
    """What SdcEngine.gae hands back: `returns`, `advantages` fp32 [T, N]; `masks` fp32 [T+1, N]; `value_preds` fp32 [T+1, N] or None;
    `moments` fp64 [2] (the advantages' mean and population standard deviation) or None"""
    __slots__ = ("returns", "advantages", "masks", "value_preds", "moments")

    def __init__(self, returns, advantages, masks, value_preds, moments):
        self.returns, self.advantages, self.masks, self.value_preds, self.moments = returns, advantages, masks, value_preds, moments


class OnPolicyBatch:
    """One collected on-policy training batch on the device (SdcEngine.collect), T steps of N envs -- the reference's actor and
    critic buffers after `compute`:
      obs [T+1,N,3,26], share_obs [T+1,N,29]      row 0: what the engine held before the call, row t+1: after step t
      actions [T,N,3] int32, logits [T,N,3,3], action_log_probs [T,N,3], entropy [T,N,3]
      rewards [T,N,3], dones [T,N] uint8, masks [T+1,N] (masks[t+1] = 1 - dones[t]; masks[0] from the call's first_done)
      values [T+1,N] (the critic's, denormalised), value_preds [T+1,N] (normalised with the critic's ValueNorm: what the clipped
      value loss keeps), returns [T,N], advantages [T,N], adv_mean, adv_std (0-dim fp64), last_done [N] uint8 (the next call's
      first_done)."""
    FIELDS = ("obs", "share_obs", "actions", "logits", "action_log_probs", "entropy", "rewards", "dones", "masks", "values", "value_preds",
              "returns", "advantages", "adv_mean", "adv_std", "last_done")
    __slots__ = FIELDS

    def __init__(self, **fields):
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    @property
    def n_steps(self) -> int:
        return int(self.actions.shape[0])

    def normalized_advantages(self):
        """(advantages - adv_mean) / (adv_std + 1e-5), fp32 [T, N]: the reference's normalisation (happo.py) in one torch op"""
        t = self.advantages
        return ((t - self.adv_mean) / (self.adv_std + 1e-5)).to(t.dtype)

    def flat(self) -> dict:
        """{name: a [T*N, ...] view} of every per-step field, rows t < T of the [T+1] ones -- what a minibatch sampler indexes"""
        T = self.n_steps
        per_step = ("obs", "share_obs", "actions", "logits", "action_log_probs", "entropy", "rewards", "dones", "masks", "values",
                    "value_preds", "returns", "advantages")
        return {k: getattr(self, k)[:T].flatten(0, 1) for k in per_step}


class PPOTerms:
    """What SdcEngine.ppo_terms hands back for one agent, on the engine's device: `ratio` fp32 [T, N] (the reference's imp_weights),
    `surr` fp32 [T, N] = factor * min(ratio * A, clamp(ratio, 1 - clip, 1 + clip) * A) or None, `factor` fp32 [T, N] the UPDATED HAPPO
    factor (the one given, or ones, times ratio), `stats` fp64 [8]: the sums of surr, ratio, new - old and the entropy column, the
    number of clipped elements, the ratio's minimum and maximum, T N (include/sustaindc_hip.h states their fixed order)."""
    __slots__ = ("ratio", "surr", "factor", "stats")

    def __init__(self, ratio, surr, factor, stats):
        self.ratio, self.surr, self.factor, self.stats = ratio, surr, factor, stats

    def summary(self) -> dict:
        """The update's logged scalars, from one device -> host copy of `stats`: policy_loss = -mean(surr) (happo.py's
        policy_action_loss), ratio_mean / ratio_min / ratio_max, approx_kl = -mean(new - old), entropy (the mean of the entropy column;
        0 where none was given), clip_frac"""
        s = self.stats.cpu().numpy()
        n = float(s[7])
        return dict(policy_loss=-float(s[0]) / n, ratio_mean=float(s[1]) / n, ratio_min=float(s[5]), ratio_max=float(s[6]),
                    approx_kl=-float(s[2]) / n, entropy=float(s[3]) / n, clip_frac=float(s[4]) / n)


class _ParamGrads:
    """What ActorGrads and CriticGrads share: `flat`, the fp32 gradient with respect to a params struct's float members in
    declaration order (torch's [out][in] layout), and `sq_norm` fp64 0-dim, the sum of its squares in the fixed order
    include/sustaindc_hip.h states.  A subclass names its network (`_WHAT`) and gives `_layout()`: (the struct's {field: shape}, the
    reference's {field: state_dict key}, {field: the shape under that key, where it differs})."""
    __slots__ = ("flat", "sq_norm")
    _WHAT = ""

    def __init__(self, flat, sq_norm):
        self.flat, self.sq_norm = flat, sq_norm

    @staticmethod
    def _layout():
        raise NotImplementedError

    def named(self) -> dict:
        """{params struct field: a shaped view of `flat`}"""
        out, at = {}, 0
        for field, shape in self._layout()[0].items():
            n = int(np.prod(shape))
            out[field] = self.flat[at:at + n].view(shape)
            at += n
        return out

    def state_dict(self) -> dict:
        """the same views under the reference's state_dict keys, in its shapes"""
        _, keys, shapes = self._layout()
        return {keys[k]: (v.view(shapes[k]) if k in shapes else v) for k, v in self.named().items()}

    def norm(self):
        """the gradient's 2-norm, fp64 0-dim on the device"""
        return self.sq_norm.sqrt()

    def clip_(self, max_norm: float):
        """torch's clip_grad_norm_ rule on `flat`, in place: flat *= min(1, max_norm / (norm + 1e-6)); -> the norm before clipping.
        (sq_norm is left as the call computed it.)"""
        total = self.norm()
        self.flat.mul_((float(max_norm) / (total + 1e-6)).clamp(max=1.0).to(self.flat.dtype))
        return total

    def assign_to(self, module):
        """.grad of every parameter of `module` that has the reference's keys (a module without a feature_norm takes the rest)"""
        sd = self.state_dict()
        for name, p in module.named_parameters():
            if name not in sd:
                raise KeyError(f"assign_to: the module's parameter {name!r} is none of the {self._WHAT}'s {sorted(sd)}")
            p.grad = sd[name].detach().to(device=p.device, dtype=p.dtype).clone()


class ActorGrads(_ParamGrads):
    """What SdcEngine.actor_backward hands back for one agent, on the engine's device: `flat` fp32 [6391], the gradient with respect to
    the float members of sdc_actor_params in declaration order (ln0_gamma .. b3, torch's [out][in] layout), and `sq_norm` fp64 0-dim,
    the sum of its squares in the fixed order include/sustaindc_hip.h states.  state_dict(): the reference's StochasticPolicy keys."""
    __slots__ = ()
    _WHAT = "actor"

    @staticmethod
    def _layout():
        return _ACTOR_SHAPES, _ACTOR_SD_KEYS, {}


class CriticGrads(_ParamGrads):
    """What SdcEngine.critic_backward hands back, on the engine's device: `flat` fp32 [6459], the gradient with respect to the float
    members of sdc_critic_params from ln0_g to b3 in declaration order (scale and shift are no parameters), and `sq_norm` fp64 0-dim.
    state_dict(): the reference's VNet keys, v_out.weight as [1, 64] and v_out.bias as [1]."""
    __slots__ = ()
    _WHAT = "critic"

    @staticmethod
    def _layout():
        return _CRITIC_SHAPES, _CRITIC_SD_KEYS, {"w3": (1, 64), "b3": (1,)}


class ValueLossTerms:
    """What SdcEngine.value_loss hands back, on the engine's device: `loss` fp32 (the inputs' shape; None without want_loss) the value
    loss per element, `dvalue` fp32 the derivative of coef * sum(loss) per raw value -- critic_backward's coefficients --, `stats` fp64
    [8]: the sums of loss, the raw values, the error target - raw and its square, the number of elements whose clipped loss is the
    larger, the error's minimum and maximum, n (include/sustaindc_hip.h states their fixed order)."""
    __slots__ = ("loss", "dvalue", "stats")

    def __init__(self, loss, dvalue, stats):
        self.loss, self.dvalue, self.stats = loss, dvalue, stats

    def summary(self) -> dict:
        """The update's logged scalars, from one device -> host copy of `stats`: value_loss = mean(loss) (v_critic.py's value_loss),
        value_mean (of the raw values), error_mean, error_rms, clipped_frac, error_min, error_max"""
        s = self.stats.cpu().numpy()
        n = float(s[7])
        return dict(value_loss=float(s[0]) / n, value_mean=float(s[1]) / n, error_mean=float(s[2]) / n,
                    error_rms=float(np.sqrt(float(s[3]) / n)), clipped_frac=float(s[4]) / n, error_min=float(s[5]), error_max=float(s[6]))


class MiniBatch(OnPolicyBatch):
    """What SdcEngine.minibatch hands back: an OnPolicyBatch of T' = len(indices) / N steps whose per-step fields are the parent's rows
    `indices`, every field [T', N, ...] (there is no row T').  A field the call was told not to gather is None; with `agent` given the
    other agents' columns of the per-agent fields hold anything.  adv_mean, adv_std and last_done are the parent's.  `factor`: the
    gathered HAPPO factor [T', N] or None; `bad`: int32 [1], 1 when an index lay outside the parent's rows (that row is zeros)."""
    __slots__ = ("factor", "bad", "_steps")

    def __init__(self, steps, factor=None, bad=None, **fields):
        super().__init__(**fields)
        self.factor, self.bad, self._steps = factor, bad, int(steps)

    @property
    def n_steps(self) -> int:
        return self._steps


class TrainInfo:
    """What SdcEngine.happo_train hands back, everything on the device: `actor[a]`, the (PPOTerms.stats fp64 [8], gradient norm fp64
    0-dim) of every update of agent a in the order they ran; `critic`, the (ValueLossTerms.stats, gradient norm) of every critic
    update; `factor` fp32 [T, N], the HAPPO factor behind the last agent (None without use_factor)."""
    __slots__ = ("actor", "critic", "factor")

    def __init__(self):
        self.actor, self.critic, self.factor = {}, [], None

    def summary(self) -> dict:
        """The reference's train_info, the means over a network's updates, from ONE device -> host copy: {"actor": {agent:
        {policy_loss, dist_entropy, actor_grad_norm, ratio}}, "critic": {value_loss, critic_grad_norm}}"""
        import torch
        groups = [(a, self.actor[a]) for a in sorted(self.actor)] + [("critic", self.critic)]
        rows = [torch.cat((stats, norm.reshape(1))) for _, ups in groups for stats, norm in ups]
        if not rows:
            return {"actor": {}, "critic": {}}
        host = torch.stack(rows).cpu().numpy()
        out, at = {"actor": {}, "critic": {}}, 0
        for who, ups in groups:
            s = host[at:at + len(ups)]
            at += len(ups)
            if not len(ups):
                continue
            n = s[:, 7]
            if who == "critic":
                out["critic"] = dict(value_loss=float(np.mean(s[:, 0] / n)), critic_grad_norm=float(np.mean(s[:, 8])))
            else:
                out["actor"][who] = dict(policy_loss=float(np.mean(-s[:, 0] / n)), dist_entropy=float(np.mean(s[:, 3] / n)),
                                         actor_grad_norm=float(np.mean(s[:, 8])), ratio=float(np.mean(s[:, 1] / n)))
        return out


class MPCCarry:
    """What `rollout_cem_stats` leaves of the planner's state, on the engine's device: `probs` float64 [H, N, 3, 3] and `best_seq` int32
    [H, N, 3], the arrays of the call (a caller's own are the same tensors), whose first `steps` steps hold the last planned decision's
    result, unshifted -- `steps` is 0 when no decision of the call was planned or its last one was idle: nothing to resume from --;
    `planned`: the number of planned decisions of the call (what the draw counter advances by); `best_action` int32 [N, 3] the last
    action played; `best_score` float64 [I, N] the last planned decision's scores.  From `rollout_cem_groups_stats` the arrays are per
    group -- probs [H, G, 3, 3], best_seq [H, G, 3], best_action [G, 3], best_score [I, G] -- and `step_actions` int32 [N, 3] is the last
    action played, per env (None from the per-env call)."""

    def __init__(self, probs, best_seq, steps, planned, best_action, best_score, step_actions=None):
        self.probs, self.best_seq, self.steps, self.planned = probs, best_seq, int(steps), int(planned)
        self.best_action, self.best_score, self.step_actions = best_action, best_score, step_actions


def mpc_schedule(left, n_steps, horizon, auto_reset, warm_start=True, resume_steps=0):
    """The decisions of a `rollout_cem_stats` call of n_steps that starts `left` steps before the episode's end, by the library's rule
    (csrc/sdc_mpc_schedule.hpp; agents._mpc_horizon and CEMMPCAgent._start) -> a list of (K, planned, fresh, draw index) per step."""
    out, carried, j = [], int(resume_steps), 0
    for t in range(int(n_steps)):
        lt = left - t
        K = min(horizon, lt - 1 if auto_reset else lt)
        if not (lt >= 2 and K >= 1):
            out.append((0, False, False, 0))
            carried = 0
            continue
        out.append((K, True, (not warm_start) or carried == 0 or K > carried, j))
        carried, j = K, j + 1
    return out


def _p(x):
    """a device tensor's address for the library (None stays a null pointer)"""
    return None if x is None else C.c_void_p(x.data_ptr())


def _ip(a):
    """... and a host int32 array's"""
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def plan_objective(reward_weights=(1.0, 1.0, 1.0), gamma: float = 1.0, info_weights=None) -> L.SdcPlanObjective:
    """plan's objective as the library's struct; ValueError for anything but three reward weights, an unknown info key, more than
    PLAN_MAX_COLS keys (gamma is the library's to refuse)."""
    w = [float(x) for x in reward_weights]
    if len(w) != 3:
        raise ValueError(f"plan: reward_weights must be three numbers (ls, dc, bat), got {len(w)}")
    cols = dict(info_weights or {})
    if len(cols) > L.PLAN_MAX_COLS:
        raise ValueError(f"plan: info_weights names {len(cols)} keys, at most {L.PLAN_MAX_COLS} can be weighed")
    o = L.SdcPlanObjective()
    o.reward_weight[:] = w
    o.gamma = float(gamma)
    o.n_cols = len(cols)
    for j, (key, weight) in enumerate(cols.items()):
        if key not in L.INFO_IDX:
            raise ValueError(f"plan: info_weights key {key!r} is not an info column (dc_rl_amd._lib.INFO_COLS)")
        o.col[j] = L.INFO_IDX[key]
        o.col_weight[j] = float(weight)
    return o


def dc_params_struct(p: dict) -> L.SdcDcParams:
    """dict (see dc_config.size_datacenter) -> C struct."""
    s = L.SdcDcParams()
    R = len(p["rack_n"])
    if not 1 <= R <= L.MAX_RACKS:
        raise ValueError(f"n_racks must be in [1, {L.MAX_RACKS}], got {R}")
    s.n_racks = R
    for name in ("rack_n", "rack_full", "rack_idle", "rack_supply", "rack_return"):
        dst = getattr(s, name)
        src = p[name]
        if len(src) != R:
            raise ValueError(f"{name} has {len(src)} entries, expected {R}")
        for i in range(R):
            dst[i] = float(src[i])
    for name in ("m_cpu", "c_cpu", "rs_cpu", "m_fan", "c_fan", "rs_fan", "itfan_ref_p", "itfan_ref_v_ratio",
                 "it_fan_full_load_v", "c_air", "rho_air", "crac_supply_pu", "ct_fan_ref_p", "ctafr", "min_temp",
                 "max_temp"):
        setattr(s, name, float(p[name]))
    s.init_setpoint = float(p.get("init_setpoint", 18.0))
    s.bat_capacity_mwh = float(p["bat_capacity"])
    return s


_ACTOR_SD_KEYS = {   # the reference's StochasticPolicy state_dict -> sdc_actor_params fields
    "ln0_gamma": "base.feature_norm.weight", "ln0_beta": "base.feature_norm.bias",
    "w1": "base.mlp.fc.0.weight", "b1": "base.mlp.fc.0.bias", "ln1_gamma": "base.mlp.fc.2.weight", "ln1_beta": "base.mlp.fc.2.bias",
    "w2": "base.mlp.fc.3.weight", "b2": "base.mlp.fc.3.bias", "ln2_gamma": "base.mlp.fc.5.weight", "ln2_beta": "base.mlp.fc.5.bias",
    "w3": "act.action_out.linear.weight", "b3": "act.action_out.linear.bias",
}
_ACTOR_SHAPES = {"ln0_gamma": (26,), "ln0_beta": (26,), "w1": (64, 26), "b1": (64,), "ln1_gamma": (64,), "ln1_beta": (64,),
                 "w2": (64, 64), "b2": (64,), "ln2_gamma": (64,), "ln2_beta": (64,), "w3": (3, 64), "b3": (3,)}


def actor_params(params) -> L.SdcActorParams:
    """dict (sdc_actor_params field names, or the reference's StochasticPolicy state_dict keys) -> C struct."""
    p = L.SdcActorParams()
    feature_norm = True
    for field, shape in _ACTOR_SHAPES.items():
        v = params.get(field, params.get(_ACTOR_SD_KEYS[field]))
        if v is None:
            if field in ("ln0_gamma", "ln0_beta"):      # use_feature_normalization False: no feature_norm in the state_dict
                feature_norm = False
                continue
            raise KeyError(f"actor parameters: neither {field!r} nor {_ACTOR_SD_KEYS[field]!r} given")
        a = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"actor parameter {field}: shape {a.shape}, expected {shape} (hidden_sizes [64, 64], 26 inputs, 3 actions)")
        C.memmove(getattr(p, field), a.ctypes.data, a.nbytes)
    p.use_feature_normalization = 1 if params.get("use_feature_normalization", feature_norm) else 0
    act = params.get("activation", "tanh")
    if act not in ("tanh", "relu", 0, 1):
        raise NotImplementedError(f"actor activation {act!r}: the kernel runs tanh (happo.yaml) and relu")
    p.activation = {"tanh": 0, "relu": 1}.get(act, act)
    return p


_CRITIC_SD_KEYS = {   # the reference's VNet state_dict -> sdc_critic_params fields
    "ln0_g": "base.feature_norm.weight", "ln0_b": "base.feature_norm.bias",
    "w1": "base.mlp.fc.0.weight", "b1": "base.mlp.fc.0.bias", "ln1_g": "base.mlp.fc.2.weight", "ln1_b": "base.mlp.fc.2.bias",
    "w2": "base.mlp.fc.3.weight", "b2": "base.mlp.fc.3.bias", "ln2_g": "base.mlp.fc.5.weight", "ln2_b": "base.mlp.fc.5.bias",
    "w3": "v_out.weight", "b3": "v_out.bias",
}
_CRITIC_SHAPES = {"ln0_g": (29,), "ln0_b": (29,), "w1": (64, 29), "b1": (64,), "ln1_g": (64,), "ln1_b": (64,),
                  "w2": (64, 64), "b2": (64,), "ln2_g": (64,), "ln2_b": (64,), "w3": (64,), "b3": ()}


def _struct_state_dict(p, shapes, keys, sd_shapes, feature_norm):
    """a params struct's float members under the reference's state_dict keys, as torch tensors on the host (copies); without the
    feature LayerNorm's two when it is off, as the reference's module has none then"""
    import torch
    out = {}
    for field, shape in shapes.items():
        if not feature_norm and field.startswith("ln0_"):
            continue
        v = getattr(p, field)
        a = np.array(v, dtype=np.float32) if isinstance(v, float) else np.ctypeslib.as_array(v).astype(np.float32, copy=True)
        out[keys[field]] = torch.from_numpy(a.reshape(sd_shapes.get(field, shape)).copy())
    return out


def value_norm_scale_shift(value_norm):
    """A ValueNorm folded into (scale, shift) of `value * scale + shift`, in fp32 as harl/common/valuenorm.py running_mean_var and
    denormalize do it: None -> (1, 0); a (mean, var) pair -> (sqrt(var), mean); an object or dict with running_mean, running_mean_sq
    and debiasing_term -> the debiased mean and variance first (the debiasing term clamped at 1e-5, the variance at 1e-2)."""
    f = np.float32
    if value_norm is None:
        return 1.0, 0.0
    get = (lambda k: value_norm[k]) if isinstance(value_norm, dict) else (lambda k: getattr(value_norm, k))
    num = lambda v: f(np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32).reshape(-1)[0])
    if isinstance(value_norm, (tuple, list)):
        if len(value_norm) != 2:
            raise ValueError("critic_params: value_norm must be None, a (mean, var) pair, or hold running_mean, running_mean_sq and debiasing_term")
        mean, var = num(value_norm[0]), num(value_norm[1])
    else:
        try:
            rm, rsq, deb = num(get("running_mean")), num(get("running_mean_sq")), num(get("debiasing_term"))
        except (KeyError, AttributeError):
            raise KeyError("critic_params: value_norm holds no running_mean / running_mean_sq / debiasing_term (a ValueNorm moved across "
                           "devices drops them from its state_dict: pass the object)") from None
        deb = np.maximum(deb, f(1e-5))
        mean, mean_sq = f(rm / deb), f(rsq / deb)
        var = np.maximum(f(mean_sq - f(mean * mean)), f(1e-2))
    return float(np.sqrt(f(var))), float(mean)


def critic_params(params, value_norm=None, activation="tanh") -> L.SdcCriticParams:
    """The V critic as the library's struct.  `params`: a state_dict of the reference's VNet (harl/models/value_function_models/v_net.py:
    keys base.feature_norm.* -- absent: use_feature_normalization off --, base.mlp.fc.{0,2,3,5}.*, v_out.*; tensors or arrays), or a dict
    of the fields of sdc_critic_params (w3 [64] or [1, 64]; optionally "scale", "shift", "flags" or "activation" /
    "use_feature_normalization").  `value_norm`: see value_norm_scale_shift.  `activation`: "tanh" or "relu".  KeyError for a missing
    parameter, ValueError for a wrong shape, NotImplementedError for another activation."""
    p = L.SdcCriticParams()
    feature_norm = True
    for field, shape in _CRITIC_SHAPES.items():
        v = params.get(field, params.get(_CRITIC_SD_KEYS[field]))
        if v is None:
            if field in ("ln0_g", "ln0_b"):      # use_feature_normalization False: no feature_norm in the state_dict
                feature_norm = False
                continue
            raise KeyError(f"critic parameters: neither {field!r} nor {_CRITIC_SD_KEYS[field]!r} given")
        a = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)
        if field in ("w3", "b3") and a.size == int(np.prod(shape, dtype=np.int64)):
            a = a.reshape(shape)                 # (v_out: Linear(64, 1) stores [1, 64] and [1])
        if a.shape != shape:
            raise ValueError(f"critic parameter {field}: shape {a.shape}, expected {shape} (hidden_sizes [64, 64], 29 inputs, one value)")
        if field == "b3":
            p.b3 = float(a)
        else:
            C.memmove(getattr(p, field), a.ctypes.data, a.nbytes)
    act = params.get("activation", activation)
    if act not in ("tanh", "relu", 0, 1):
        raise NotImplementedError(f"critic activation {act!r}: the kernel runs tanh and relu")
    p.flags = (1 if params.get("use_feature_normalization", feature_norm) else 0) | ({"tanh": 0, "relu": 1}.get(act, act) << 1)
    if "flags" in params:
        p.flags = int(params["flags"])
    scale, shift = value_norm_scale_shift(value_norm)
    p.scale, p.shift = float(params.get("scale", scale)), float(params.get("shift", shift))
    return p


class SdcEngine:
    def __init__(self, n_envs: int, episode_steps: int = 672, device: int = 0, n_locations: int = 1,
                 n_dc_configs: int = 1, auto_reset: bool = True, seed: int = 0, hist_cap: int = 10000,
                 queue_max_len: int = 1000, weather_noise_std: float = 0.75, weather_noise_weight: float = 0.02,
                 max_roll_days: int = 14, debug_flags: int = 0, reward_method=(0, 0, 0), env_index_base: int = 0,
                 policy=(0, 0, 0), trim_and_respond_limit: float = 27.0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("SdcEngine needs an MI355X visible to PyTorch-ROCm (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = L.load()
        self.torch = torch
        self.n_envs = int(n_envs)
        self.episode_steps = int(episode_steps)
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        cfg = L.SdcConfig(n_envs=self.n_envs, device=self.device_index, episode_steps=self.episode_steps,
                          hist_cap=hist_cap, queue_max_len=queue_max_len, n_locations=n_locations,
                          n_dc_configs=n_dc_configs, auto_reset=1 if auto_reset else 0, seed=seed,
                          weather_noise_std=weather_noise_std, weather_noise_weight=weather_noise_weight,
                          max_roll_days=max_roll_days, debug_flags=debug_flags,
                          reward_method=(C.c_int32 * 3)(*[int(m) for m in reward_method]),
                          env_index_base=int(env_index_base), policy=(C.c_int32 * 3)(*[int(x) for x in policy]),
                          trim_and_respond_limit=float(trim_and_respond_limit))
        self.policy = tuple(int(x) for x in policy)
        # the sdc_config fields a checkpoint records (all but device and debug_flags: where and how it runs, not what it is)
        self.config = dict(n_envs=self.n_envs, episode_steps=self.episode_steps, hist_cap=int(hist_cap),
                           queue_max_len=int(queue_max_len), n_locations=int(n_locations), n_dc_configs=int(n_dc_configs),
                           auto_reset=bool(auto_reset), weather_noise_std=float(weather_noise_std),
                           weather_noise_weight=float(weather_noise_weight), max_roll_days=int(max_roll_days),
                           reward_method=tuple(int(m) for m in reward_method), env_index_base=int(env_index_base),
                           policy=self.policy, trim_and_respond_limit=float(trim_and_respond_limit))
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._h = C.c_void_p()
        self._pinned_stream = None
        self._pinned_stream_obj = None
        self._out_ptrs = None
        self._done_buf = None
        self._forecast_values = None      # set_plan_forecast's `values`, kept alive while the library holds its address
        self._actors = {}                 # set_actor's structs by slot; the slots of _stale_actors have been stepped on the device since
        self._critic = None               # set_critic's struct (_stale_critic likewise): _host_actors() / _host_critic() refresh them
        self._stale_actors = set()
        self._stale_critic = False
        self._value_norm_installed = False      # set_value_norm: the critic's scale and shift follow a ValueNorm kept on the device
        with torch.cuda.device(self.device):
            torch.cuda.init()
            L.check(self.lib.sdc_create(C.byref(cfg), C.byref(self._h)))
        self.lw = self.lib.sdc_weather_window_len(self._h)
        self.hist_stride = self.lib.sdc_hist_stride(self._h)
        self.queue_stride = self.lib.sdc_queue_stride(self._h)
        self._sizes = dict(n_envs=self.n_envs, hist_stride=self.hist_stride, lw=self.lw, queue_stride=self.queue_stride,
                           hist_cap=int(hist_cap))
        # the step's outputs are views of ONE device allocation (the layout: _args.out_layout)
        self.out_flat = torch.zeros(A.out_layout(self.n_envs)[1], dtype=torch.uint8, device=self.device)
        self.obs, self.share_obs, self.rew, self.done, self.info = self.split_out_flat(self.out_flat)
        self.final_obs = torch.zeros((self.n_envs, L.N_AGENTS, L.OBS_PAD), dtype=torch.float32, device=self.device)
        self._all_envs = np.arange(self.n_envs, dtype=np.int32)
        self._obs_ptrs = (_p(self.obs), _p(self.share_obs))      # (the pair most calls end with; the tensors live as long as the engine)

    # ------------------------------------------------------------------ the call into the library (all but step()'s)
    def _call(self, fn, *args, refuses=False, wrote=()):
        """fn(handle, *args) on the engine's device.  A return code other than 0 raises what the entry point always raised: SdcError
        (the older ones), or -- `refuses` -- ValueError for a refusal (rc -2: nothing reached the device) and SdcError for the rest.
        `wrote`: the tensors (None: skipped) the call wrote or read on the launch stream; they are record_stream'ed when it is pinned."""
        with self.torch.cuda.device(self.device):
            rc = fn(self._h, *args)
        if refuses:
            self._refused(rc)
        elif rc != 0:
            L.check(rc)
        if self._pinned_stream_obj is not None:      # (used on the pinned stream: the allocator must not reuse them before)
            for x in wrote:
                if x is not None:
                    x.record_stream(self._pinned_stream_obj)

    def _refused(self, rc):
        if rc == -2:        # (a refusal: fail_msg, before anything reached the device)
            raise ValueError(self.lib.sdc_last_error().decode())
        L.check(rc)

    def _behind_torch_stream(self):
        """tensors filled by torch ops on torch's current stream are about to be read by a kernel on the pinned one: order it behind them"""
        if self._pinned_stream_obj is not None:
            self._pinned_stream_obj.wait_stream(self.torch.cuda.current_stream(self.device))

    def _identity(self):
        """what this engine is: its configuration and the library's state layout (what checkpoints and snapshots are held to)"""
        return dict(self.config, layout=int(self.lib.sdc_state_layout()))

    # ------------------------------------------------------------------ setup
    def set_tables(self, loc_id: int, W, Cc, T, WB):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (W, Cc, T, WB)]
        for a in arrs:
            if a.shape != (L.TABLE_LEN,):
                raise ValueError(f"trace tables must have shape ({L.TABLE_LEN},), got {a.shape}")
        dp = C.POINTER(C.c_double)
        self._call(self.lib.sdc_set_tables, int(loc_id), *[a.ctypes.data_as(dp) for a in arrs], L.TABLE_LEN)

    def set_dc_params(self, cfg_id: int, params: dict):
        self._call(self.lib.sdc_set_dc_params, int(cfg_id), C.byref(dc_params_struct(params)))

    def assign(self, loc_id, cfg_id, day_lo, day_hi):
        N = self.n_envs
        arrs = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int32), (N,))) for a in
                (loc_id, cfg_id, day_lo, day_hi)]
        self._call(self.lib.sdc_assign_envs, *[_ip(a) for a in arrs])

    def set_seed(self, seed: int):
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._call(self.lib.sdc_set_seed, seed)
        self.seed = seed

    # ------------------------------------------------------------------ run
    def _stream(self):
        # launches go to torch's current stream, or to the stream pinned with use_stream() (an engine per env group,
        # each on its own stream, lets the groups' steps overlap: tools/two_streams.py)
        if self._pinned_stream is not None:
            return self._pinned_stream
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def use_stream(self, stream=None):
        """Pin this engine's launches to a torch.cuda.Stream (None: back to torch's current stream)."""
        self._pinned_stream = None if stream is None else C.c_void_p(stream.cuda_stream)
        self._pinned_stream_obj = stream

    def reset(self, mask: Optional[np.ndarray] = None, override: Optional[dict] = None):
        """SustainDC.reset for the masked envs (all if mask is None).  Returns (obs, share_obs) device tensors
        (views of the engine's buffers)."""
        N = self.n_envs
        mptr = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.shape != (N,):
                raise ValueError("mask must have shape (n_envs,)")
            mptr = m.ctypes.data_as(C.POINTER(C.c_uint8))
        o = None
        if override is not None:
            arrays = A.reset_override(override, self._sizes)        # (alive until the call returns: the struct holds addresses)
            o = L.SdcResetOverride(**{f: a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double))
                                      for f, a in arrays.items()})
        self._call(self.lib.sdc_reset, mptr, None if o is None else C.byref(o), *self._obs_ptrs, self._stream())
        return self.obs, self.share_obs

    def step(self, actions, want_info: bool = True):
        """actions: int32 device tensor [N, 3] (ls, dc, bat).  Returns views of the engine's buffers:
        obs [N,3,26], share_obs [N,29], rew [N,3], done [N] (uint8), info [N,40]."""
        t = self.torch
        if actions is None:
            if any(p == 0 for p in self.policy):
                raise ValueError("actions=None needs a built-in policy on every agent slot (SdcEngine(policy=...))")
        elif not (isinstance(actions, t.Tensor) and actions.dtype == t.int32 and actions.is_cuda and
                  actions.is_contiguous() and tuple(actions.shape) == (self.n_envs, 3)):
            raise ValueError("actions must be a contiguous int32 CUDA tensor of shape (n_envs, 3)")
        p = self._out_ptrs
        if p is None:   # the output tensors live as long as the engine: take their addresses once
            p = self._out_ptrs = tuple(C.c_void_p(x.data_ptr()) for x in
                                       (self.obs, self.share_obs, self.rew, self.done, self.info, self.final_obs))
        args = (self._h, C.c_void_p(actions.data_ptr()) if actions is not None else None, p[0], p[1], p[2], p[3],
                p[4] if want_info else None, p[5],
                self._stream())
        if t.cuda.current_device() == self.device_index:   # the usual case (one process per GPU): no device switch
            rc = self.lib.sdc_step(*args)
        else:
            with t.cuda.device(self.device):
                rc = self.lib.sdc_step(*args)
        if rc != 0:
            L.check(rc)
        return self.obs, self.share_obs, self.rew, self.done, self.info

    def split_out_flat(self, flat):
        """Views (obs, share_obs, rew, done, info) over a host / device copy of `out_flat` (a uint8 tensor of the same size)."""
        v = A.out_views(flat, self.n_envs)
        return v["obs"], v["share"], v["rew"], v["done"], v["info"]

    def last_step_kernel(self) -> str:
        """Name of the step kernel the last `step()` launched (the host picks by batch size and configuration; all give the same
        results)."""
        return self.lib.sdc_last_step_kernel(self._h).decode()

    def last_done(self):
        """bool [N]: which envs finished in the last step() / rollout() -- from the host's mirror of the step counters, no
        device synchronisation.  None when no env finished."""
        if self._done_buf is None:
            self._done_buf = np.zeros(self.n_envs, dtype=np.uint8)
            self._done_ptr = self._done_buf.ctypes.data_as(C.POINTER(C.c_uint8))
        n = self.lib.sdc_last_done(self._h, self._done_ptr)
        if n < 0:
            L.check(n)
        return self._done_buf.astype(bool) if n > 0 else None

    def steps_to_episode_end(self) -> int:
        return int(self.lib.sdc_steps_to_episode_end(self._h))

    def rollout_policy(self, n_steps: int, actions=None, want_info: bool = True):
        """`rollout` for engines whose agent slots (some or all) are played by built-in policies (`policy=`): closed-loop
        episodes at rollout speed.  actions: None when every slot has a policy, else [K, N, 3] (slots with a policy
        ignore their column).  Returns (obs, share_obs, rew, done, info, actions_applied [K, N, 3] int32)."""
        return self.rollout(actions, want_info=want_info, n_steps=n_steps, want_actions=True)

    def rollout(self, actions, want_info: bool = True, n_steps: int = None, want_actions: bool = False):
        """K env-steps in one launch for an action sequence known up front (scripted / rule-based policies, open-loop
        evaluation).  actions: int32 device tensor [K, N, 3]; K must not run past the end of an episode
        (steps_to_episode_end()).  Returns fresh device tensors holding every step's outputs:
        obs [K,N,3,26], share_obs [K,N,29], rew [K,N,3], done [K,N] (uint8), info [K,N,44] (or None).
        Same results as K calls of step()."""
        t = self.torch
        K = self._sequence_steps("", actions, n_steps)     # (no device check: DESIGN.md 4.18, kept oddities)
        out = self._rollout_outputs(K, want_info)
        aout = t.empty((K, self.n_envs, 3), dtype=t.int32, device=self.device) if want_actions else None
        self._call(self.lib.sdc_rollout, K, _p(actions), *[_p(x) for x in out], _p(self.final_obs), _p(aout), self._stream(),
                   wrote=out + (aout,))
        self._views_follow(*out)
        return out + (aout,) if want_actions else out

    def _sequence_steps(self, who, actions, n_steps, device=None):
        """K of rollout's and rollout_stats' arguments: an action sequence [K, N, 3] (on `device`, if given), or None with n_steps when
        every slot has a built-in policy; ValueError in `who`'s name ("": none) for anything else"""
        pre = f"{who}: " if who else ""
        if actions is None:
            if n_steps is None or any(p == 0 for p in self.policy):
                raise ValueError(f"{pre}actions=None needs n_steps and a built-in policy on every agent slot")
            return int(n_steps)
        A.device_tensor(actions, who, "actions", self.torch.int32, (A.ANY, self.n_envs, 3), "(K, n_envs, 3)", device, True)
        if n_steps is not None and int(n_steps) != int(actions.shape[0]):
            raise ValueError(f"{pre}n_steps does not match the action sequence")
        return int(actions.shape[0])

    def _rollout_outputs(self, K, want_info=True):
        """fresh tensors for K steps' outputs: (obs, share_obs, rew, done, info or None)"""
        t, N = self.torch, self.n_envs
        new = lambda shape, dtype=t.float32: t.empty((K, N) + shape, dtype=dtype, device=self.device)
        return (new((L.N_AGENTS, L.OBS_PAD)), new((L.SHARE_OBS_DIM,)), new((L.N_AGENTS,)), new((), t.uint8),
                new((L.INFO_DIM,)) if want_info else None)

    def _views_follow(self, *out):
        """the engine's single-step views follow the last step of a rollout's outputs (_rollout_outputs' order)"""
        for mine, x in zip((self.obs, self.share_obs, self.rew, self.done, self.info), out):
            if x is not None:
                mine.copy_(x[-1])

    # ------------------------------------------------------------------ closed loop: the actors inside the kernel
    def set_actor(self, agent_slot: int, params):
        """One agent's actor network (slot 0 agent_ls, 1 agent_dc, 2 agent_bat) for rollout_actor().  `params`: a
        state_dict of the reference's StochasticPolicy (harl/models/policy_models/stochastic_policy.py: keys
        base.feature_norm.*, base.mlp.fc.{0,2,3,5}.*, act.action_out.linear.*; tensors or arrays) or a dict with the
        fields of sdc_actor_params; `activation`: "tanh" (happo.yaml) or "relu"."""
        self._set_actor_struct(int(agent_slot), actor_params(params))

    def _set_actor_struct(self, slot: int, p: L.SdcActorParams):
        self._call(self.lib.sdc_set_actor, slot, C.byref(p))
        self._actors[slot] = p      # (the host copy: what a copy of this engine is given, SustainDCVecEnv._take_state)
        self._stale_actors.discard(slot)

    def rollout_actor(self, n_steps: int, sample: bool = False, want_logits: bool = False, want_values: bool = False):
        """K env-steps in ONE launch with the three actors (set_actor) choosing every action inside the kernel from the
        step's own observations -- the closed loop observation -> actor -> action -> step without a launch per step.
        sample=False: the distributions' mode (the reference's deterministic=True), True: a draw.
        Returns (obs [K,N,3,26], share_obs [K,N,29], rew [K,N,3], done [K,N], info [K,N,44], actions [K,N,3] int32,
        logits [K,N,3,3] or None).  K must not run past the end of the episode (steps_to_episode_end()).
        want_values=True appends values [K,N]: the critic's (set_critic) value of every returned share_obs row, one
        `critic_values` launch behind the rollout -- what a policy-gradient batch needs next to the rest."""
        t = self.torch
        K, N = int(n_steps), self.n_envs
        out = self._rollout_outputs(K)
        acts = t.empty((K, N, 3), dtype=t.int32, device=self.device)
        logits = t.empty((K, N, 3, 3), dtype=t.float32, device=self.device) if want_logits else None
        self._rollout_actor_into(K, sample, out, acts, logits)
        if want_values:
            return out + (acts, logits, self.critic_values(out[1]))
        return out + (acts, logits)

    def _rollout_actor_into(self, K, sample, out, acts, logits):
        """sdc_rollout_actor of K steps into `out` (_rollout_outputs' order), `acts` and `logits` (or None): tensors or slices of [K, ...]"""
        self._call(self.lib.sdc_rollout_actor, K, 1 if sample else 0, *[_p(x) for x in out], _p(self.final_obs), _p(acts), _p(logits),
                   self._stream(), wrote=out + (acts, logits))
        self._views_follow(*out)

    # ------------------------------------------------------------------ the critic: values, and the planners' terminal value
    def set_critic(self, params, value_norm=None, activation="tanh"):
        """The V critic for critic_values(), rollout_actor(want_values=True) and the planners' terminal value (set_plan_critic):
        `params`, `value_norm` and `activation` as `critic_params` takes them (a VNet state_dict or the fields of sdc_critic_params;
        None, a (mean, var) pair or a ValueNorm; "tanh" or "relu").  The call waits for the device (a launch in flight may read the
        critic set before).  ValueError, with the critic set before still in force, for what the library refuses: an entry that is not
        finite, scale <= 0, unknown flag bits."""
        self._set_critic_struct(critic_params(params, value_norm, activation))

    def _set_critic_struct(self, p: L.SdcCriticParams):
        self._call(self.lib.sdc_set_critic, C.byref(p), refuses=True)
        self._critic = p      # (the host copy: what a copy of this engine is given, SustainDCVecEnv._take_state)
        self._stale_critic = False
        self._value_norm_installed = False      # (the library uninstalls: scale and shift were set by hand)

    def critic_values(self, share_obs):
        """The critic's value of every row of `share_obs`, a contiguous fp32 tensor [..., 29] on this engine's device -> fp32 [...]
        (sdc_critic_values: one launch, stream-ordered; a row's value depends on that row alone).  ValueError for another tensor, an
        empty one, and before set_critic."""
        t = self.torch
        if not (isinstance(share_obs, t.Tensor) and share_obs.dtype == t.float32 and share_obs.is_cuda and share_obs.is_contiguous() and
                share_obs.dim() >= 1 and share_obs.shape[-1] == L.SHARE_OBS_DIM):
            raise ValueError(f"critic_values: share_obs must be a contiguous float32 CUDA tensor of shape (..., {L.SHARE_OBS_DIM})")
        if share_obs.device != self.device:
            raise ValueError(f"critic_values: share_obs is on {share_obs.device}, this engine runs on {self.device}")
        values = t.empty(share_obs.shape[:-1], dtype=t.float32, device=self.device)
        self._behind_torch_stream()
        self._call(self.lib.sdc_critic_values, _p(share_obs), values.numel(), _p(values), self._stream(), refuses=True,
                   wrote=(share_obs, values))
        return values

    def set_plan_critic(self, weight: float):
        """The critic (set_critic) as the planners' terminal value, kept on the engine next to the plan terms (sdc_set_plan_critic):
        while `weight` is not 0, every later `plan`, `plan_cem` and `plan_cem_groups` -- and `rollout_cem_stats` /
        `rollout_cem_groups_stats`, whose predicted score then includes it -- adds gamma ** K * weight * V(share_obs after the horizon's
        last step) to a candidate's score, 0 where that step ended the episode; `returns` never see it (the exact operation order:
        include/sustaindc_hip.h).  One more launch per candidate.  0 (the default) turns it off: nothing is launched and every
        result is what it is without a critic.  Host state: nothing is enqueued.  ValueError for a weight that is not finite, and for
        a weight other than 0 before set_critic."""
        self._call(self.lib.sdc_set_plan_critic, float(weight), refuses=True)

    @property
    def plan_critic(self) -> float:
        """The plan critic's weight in force, read back from the library (0.0: off)"""
        w = C.c_double()
        self._call(self.lib.sdc_get_plan_critic, C.byref(w), refuses=True)
        return w.value

    # ------------------------------------------------------------------ the on-policy batch: log-probs, GAE, collect
    def action_log_probs(self, actions, logits, want_entropy: bool = True):
        """The log-probability of every action played and the entropy of its distribution (sdc_action_log_probs: one launch,
        stream-ordered; fp64 arithmetic rounded once to fp32, as rollout_actor_stats' sums): `actions` int32 [T, N, 3] and `logits`
        fp32 [T, N, 3, 3], contiguous on this engine's device -> (log_probs [T, N, 3], entropy [T, N, 3] or None)."""
        t, who, N = self.torch, "action_log_probs", self.n_envs
        A.device_tensor(actions, who, "actions", t.int32, (A.SOME, N, 3), "(T, n_envs, 3)", self.device)
        T = int(actions.shape[0])
        A.device_tensor(logits, who, "logits", t.float32, (T, N, 3, 3), "(T, n_envs, 3, 3)", self.device)
        logp = t.empty((T, N, 3), dtype=t.float32, device=self.device)
        ent = t.empty((T, N, 3), dtype=t.float32, device=self.device) if want_entropy else None
        self._behind_torch_stream()
        self._call(self.lib.sdc_action_log_probs, T, _p(actions), _p(logits), _p(logp), _p(ent), self._stream(), refuses=True,
                   wrote=(actions, logits, logp, ent))
        return logp, ent

    def gae(self, rew, done, values, gamma: float = 0.99, gae_lambda: float = 0.95, use_gae: bool = True, reward_agent: int = 0,
            first_done=None, want_value_preds: bool = False, want_moments: bool = True) -> GAEResult:
        """Returns, advantages and masks of a collected rollout (sdc_gae: the reference's compute_returns in its own fp32 order, one
        lane per env, stream-ordered): `rew` fp32 [T, N, 3] (column `reward_agent` is read), `done` uint8 [T, N], `values` fp32
        [T+1, N] (denormalised; row T the bootstrap), `first_done` uint8 [N] or None, all contiguous on this engine's device.
        `want_value_preds`: also (values - shift) / scale with the critic's (set_critic) ValueNorm; `want_moments`: also the advantages'
        mean and population standard deviation in fp64.  ValueError for another tensor and for what the library refuses (gamma or
        gae_lambda outside [0, 1], reward_agent outside 0..2, value_preds before set_critic)."""
        t, who, N = self.torch, "gae", self.n_envs
        A.device_tensor(rew, who, "rew", t.float32, (A.SOME, N, 3), "(T, n_envs, 3)", self.device)
        T = int(rew.shape[0])
        A.device_tensor(done, who, "done", t.uint8, (T, N), "(T, n_envs)", self.device)
        A.device_tensor(values, who, "values", t.float32, (T + 1, N), "(T + 1, n_envs)", self.device)
        if first_done is not None:
            A.device_tensor(first_done, who, "first_done", t.uint8, (N,), "(n_envs,)", self.device)
        new = lambda rows, dtype=t.float32: t.empty((rows, N), dtype=dtype, device=self.device)
        res = GAEResult(new(T), new(T), new(T + 1), new(T + 1) if want_value_preds else None,
                        t.empty(2, dtype=t.float64, device=self.device) if want_moments else None)
        self._behind_torch_stream()
        self._call(self.lib.sdc_gae, T, _p(rew), int(reward_agent), _p(done), _p(first_done), _p(values), float(gamma), float(gae_lambda),
                   int(use_gae), _p(res.returns), _p(res.advantages), _p(res.masks), _p(res.value_preds), _p(res.moments), self._stream(),
                   refuses=True, wrote=(rew, done, first_done, values, res.returns, res.advantages, res.masks, res.value_preds, res.moments))
        return res

    def collect(self, n_steps: int, gamma: float = 0.99, gae_lambda: float = 0.95, sample: bool = True, use_gae: bool = True,
                reward_agent: int = 0, first_done=None) -> OnPolicyBatch:
        """The collection phase of the reference's on-policy runner, on the device: `n_steps` env-steps played by the three actors
        (set_actor; `sample` as rollout_actor's) -> an OnPolicyBatch.  The batch's tensors are allocated once; the steps run as
        `rollout_actor` launches of steps_to_episode_end() steps at most, each into its slice of them, so n_steps may cross episode
        ends under auto-reset (the row after a done step is then the new episode's observation); then one `critic_values` launch over
        all (T+1) N share_obs rows, `action_log_probs`, and `gae` with the critic's value predictions and the moments.  Row 0 of obs /
        share_obs is what the engine held before the call; `first_done`: the last_done of the batch before (None: masks[0] = 1).
        ValueError before anything is launched: an actor or the critic missing, no episode running (no reset yet, or auto_reset off and
        the episode over), n_steps < 1, auto_reset off and n_steps past the episode's end."""
        t, N, T = self.torch, self.n_envs, int(n_steps)
        if T < 1:
            raise ValueError(f"collect: n_steps = {n_steps} must be positive")
        if len(self._actors) < 3:
            raise ValueError("collect: set_actor all three agents first")
        if self._critic is None:
            raise ValueError("collect: set_critic first")
        left = self.steps_to_episode_end()
        if left <= 0:
            raise ValueError("collect: no episode is running: call reset() first")
        if not self.config["auto_reset"] and T > left:
            raise ValueError(f"collect: n_steps = {T} would run past the end of an episode ({left} steps left; auto_reset is off)")
        if first_done is not None:
            A.device_tensor(first_done, "collect", "first_done", t.uint8, (N,), "(n_envs,)", self.device)
        new = lambda rows, shape=(), dtype=t.float32: t.empty((rows, N) + shape, dtype=dtype, device=self.device)
        obs, share = new(T + 1, (L.N_AGENTS, L.OBS_PAD)), new(T + 1, (L.SHARE_OBS_DIM,))
        rew, done = new(T, (L.N_AGENTS,)), new(T, (), t.uint8)
        acts, logits = new(T, (3,), t.int32), new(T, (3, 3))
        info = new(min(T, self.episode_steps), (L.INFO_DIM,))      # (the rollouts' info rows, one launch's at a time: not part of the batch)
        obs[0].copy_(self.obs)
        share[0].copy_(self.share_obs)
        self._behind_torch_stream()
        k = 0
        while k < T:
            K = min(T - k, self.steps_to_episode_end())
            cut = lambda x: x[k:k + K]
            self._rollout_actor_into(K, sample, (obs[1 + k:1 + k + K], share[1 + k:1 + k + K], cut(rew), cut(done), info[:K]),
                                     cut(acts), cut(logits))
            k += K
        values = self.critic_values(share)
        logp, ent = self.action_log_probs(acts, logits)
        g = self.gae(rew, done, values, gamma, gae_lambda, use_gae, reward_agent, first_done, want_value_preds=True)
        return OnPolicyBatch(obs=obs, share_obs=share, actions=acts, logits=logits, action_log_probs=logp, entropy=ent, rewards=rew,
                             dones=done, masks=g.masks, values=values, value_preds=g.value_preds, returns=g.returns,
                             advantages=g.advantages, adv_mean=g.moments[0], adv_std=g.moments[1], last_done=done[T - 1])

    # ------------------------------------------------------------------ the actors on stored rows, the PPO terms
    def _actor_evaluate(self, agent, obs, offset, row_stride, n_rows, logits, logits_offset, logits_stride):
        """sdc_actor_evaluate of `n_rows` rows of `obs` from float `offset`, `row_stride` floats apart, into `logits` likewise"""
        self._call(self.lib.sdc_actor_evaluate, agent, C.c_void_p(obs.data_ptr() + 4 * offset), row_stride, n_rows,
                   C.c_void_p(logits.data_ptr() + 4 * logits_offset), logits_stride, self._stream(), refuses=True, wrote=(obs, logits))

    def actor_logits(self, agent: int, obs, per_agent=None):
        """The logits of agent `agent`'s actor (the one last given to set_actor) for stored observation rows -- the forward pass of the
        reference's evaluate_actions, with no gradient (sdc_actor_evaluate: one launch, stream-ordered, 16 rows per wavefront on the
        matrix cores; a row's logits depend on that row alone, to the bit).  `obs`: a contiguous fp32 tensor on this engine's device,
        either (..., 26), dense rows of that agent, or (..., 3, 26), e.g. OnPolicyBatch.obs, of which the agent's rows are read in place
        (78 floats apart) -> fp32 (..., 3).  A tensor whose last but one dimension is 3 is taken as the second form; `per_agent` says
        it outright.  The envs are not touched.  ValueError for another tensor, another agent, and before set_actor(agent)."""
        t, who = self.torch, "actor_logits"
        a = A.agent_slot(who, agent)
        offset, stride, rows, shape = A.actor_rows(who, obs, a, per_agent, self.device)
        logits = t.empty(shape, dtype=t.float32, device=self.device)
        self._behind_torch_stream()
        self._actor_evaluate(a, obs, offset, stride, rows, logits, 0, 3)
        return logits

    def evaluate_actions(self, obs, actions, agents=(0, 1, 2), want_entropy: bool = True):
        """The reference's evaluate_actions over a stored batch, for the agents asked for: `obs` fp32 [T, N, 3, 26] (e.g. batch.obs[:T])
        and `actions` int32 [T, N, 3], contiguous on this engine's device -> (logits [T, N, 3, 3], log_probs [T, N, 3], entropy
        [T, N, 3] or None).  One sdc_actor_evaluate launch per agent into its column of `logits`, then one action_log_probs over all of
        it.  The columns of agents NOT asked for are zero in `logits`, and not meaningful in log_probs and entropy (they are those of
        three equal logits).  Evaluated twice with the same actors, the same rows give the same bits."""
        t, who, N = self.torch, "evaluate_actions", self.n_envs
        agents = A.agent_slots(who, agents)
        A.device_tensor(actions, who, "actions", t.int32, (A.SOME, N, 3), "(T, n_envs, 3)", self.device)
        T = int(actions.shape[0])
        A.device_tensor(obs, who, "obs", t.float32, (T, N, L.N_AGENTS, L.OBS_PAD), "(T, n_envs, 3, 26)", self.device)
        all_three = len(agents) == L.N_AGENTS
        logits = (t.empty if all_three else t.zeros)((T, N, 3, 3), dtype=t.float32, device=self.device)
        self._behind_torch_stream()
        for a in agents:
            self._actor_evaluate(a, obs, L.OBS_PAD * a, L.N_AGENTS * L.OBS_PAD, T * N, logits, 3 * a, 9)
        logp, ent = self.action_log_probs(actions, logits, want_entropy)
        return logits, logp, ent

    def ppo_terms(self, agent: int, new_log_probs, old_log_probs, advantages, clip_param: float = 0.2, factor=None, entropy=None,
                  want_surr: bool = True) -> PPOTerms:
        """What an actor update and the HAPPO factor need of one agent's log-probabilities (sdc_ppo_terms: elementwise in fp64, each
        result rounded once; fixed-order fp64 statistics; stream-ordered): `new_log_probs`, `old_log_probs` and `entropy` (or None)
        fp32 [T, N, 3], of which column `agent` is read; `advantages` and `factor` (None: ones, MAPPO) fp32 [T, N]; all contiguous on
        this engine's device -> PPOTerms: ratio = exp(new - old), surr = factor * min(ratio * A, clamp(ratio, 1 - clip, 1 + clip) * A)
        (None without `want_surr`), factor = the given factor * ratio in a new tensor, stats.  ValueError for another tensor or agent
        and for what the library refuses (clip_param outside [0, 1))."""
        t, who, N = self.torch, "ppo_terms", self.n_envs
        a = A.agent_slot(who, agent)
        A.device_tensor(new_log_probs, who, "new_log_probs", t.float32, (A.SOME, N, 3), "(T, n_envs, 3)", self.device)
        T = int(new_log_probs.shape[0])
        A.device_tensor(old_log_probs, who, "old_log_probs", t.float32, (T, N, 3), "(T, n_envs, 3)", self.device)
        A.device_tensor(advantages, who, "advantages", t.float32, (T, N), "(T, n_envs)", self.device)
        if factor is not None:
            A.device_tensor(factor, who, "factor", t.float32, (T, N), "(T, n_envs)", self.device)
        if entropy is not None:
            A.device_tensor(entropy, who, "entropy", t.float32, (T, N, 3), "(T, n_envs, 3)", self.device)
        new = lambda: t.empty((T, N), dtype=t.float32, device=self.device)
        res = PPOTerms(new(), new() if want_surr else None, new(), t.empty(L.PPO_STATS, dtype=t.float64, device=self.device))
        self._behind_torch_stream()
        self._call(self.lib.sdc_ppo_terms, T, a, _p(new_log_probs), _p(old_log_probs), _p(entropy), _p(advantages), _p(factor),
                   float(clip_param), _p(res.ratio), _p(res.surr), _p(res.factor), _p(res.stats), self._stream(), refuses=True,
                   wrote=(new_log_probs, old_log_probs, entropy, advantages, factor, res.ratio, res.surr, res.factor, res.stats))
        return res

    def actor_update_terms(self, batch, agent: int, clip_param: float = 0.2, factor=None, old_log_probs=None) -> PPOTerms:
        """The HAPPO loop's use of the two calls above for one agent of an OnPolicyBatch: `agent` is evaluated with the actor NOW set
        over batch.obs[:T] and batch.actions (evaluate_actions), and ppo_terms runs on its log-probabilities and entropies against
        `old_log_probs` (default: batch.action_log_probs, the closed loop's) and batch.normalized_advantages(), with the factor carried
        from the agents updated before (None: ones).  The runner's order -- evaluate, update the actor (set_actor), evaluate again,
        factor *= exp(new - old) -- is evaluate_actions before the update, whose log-probabilities are this call's `old_log_probs`
        after it; PPOTerms.factor is then the next agent's factor.  With the actor unchanged between the two the ratio is exactly 1."""
        a = A.agent_slot("actor_update_terms", agent)
        T = batch.n_steps
        _, logp, ent = self.evaluate_actions(batch.obs[:T], batch.actions, agents=(a,))
        old = batch.action_log_probs if old_log_probs is None else old_log_probs
        return self.ppo_terms(a, logp, old, batch.normalized_advantages(), clip_param, factor=factor, entropy=ent)

    # ------------------------------------------------------------------ the actors' gradient
    def ppo_dlogp(self, agent: int, new_log_probs, old_log_probs, advantages, clip_param: float = 0.2, factor=None, scale=None):
        """The derivative of the reference's policy loss -scale * sum(factor * min(ratio * A, clamp(ratio) * A)) with respect to each
        stored log-probability of agent `agent` (sdc_ppo_dlogp: elementwise in fp64 as ppo_terms, rounded once; stream-ordered):
        tensors as ppo_terms' -> fp32 [T, N]; zero where the clipped branch is the minimum, as torch differentiates min and clamp.
        `scale`: default 1 / (T N), the reference's mean.  ValueError for another tensor or agent and for what the library refuses."""
        t, who, N = self.torch, "ppo_dlogp", self.n_envs
        a = A.agent_slot(who, agent)
        A.device_tensor(new_log_probs, who, "new_log_probs", t.float32, (A.SOME, N, 3), "(T, n_envs, 3)", self.device)
        T = int(new_log_probs.shape[0])
        A.device_tensor(old_log_probs, who, "old_log_probs", t.float32, (T, N, 3), "(T, n_envs, 3)", self.device)
        A.device_tensor(advantages, who, "advantages", t.float32, (T, N), "(T, n_envs)", self.device)
        if factor is not None:
            A.device_tensor(factor, who, "factor", t.float32, (T, N), "(T, n_envs)", self.device)
        scale = 1.0 / (T * N) if scale is None else A.finite_float(who, "scale", scale)
        out = t.empty((T, N), dtype=t.float32, device=self.device)
        self._behind_torch_stream()
        self._call(self.lib.sdc_ppo_dlogp, T, a, _p(new_log_probs), _p(old_log_probs), _p(advantages), _p(factor), float(clip_param), scale,
                   _p(out), self._stream(), refuses=True, wrote=(new_log_probs, old_log_probs, advantages, factor, out))
        return out

    def actor_backward(self, agent: int, obs, actions, dlogp, dent: float = 0.0, per_agent=None) -> ActorGrads:
        """The gradient of L = sum_r dlogp[r] * logp_r(actions[r]) + dent * sum_r entropy_r with respect to every parameter of agent
        `agent`'s actor (the one last given to set_actor), over stored rows (sdc_actor_backward: the forward recomputed per 16-row
        tile, the backward on the matrix cores, fixed summation order: the same call gives the same bits; stream-ordered).  `obs` as
        actor_logits' (dense (..., 26) or (..., 3, 26) read in place; `per_agent` says which); `actions` int32 of the rows' shape (...)
        or (..., 3), of which the agent's column is read; `dlogp` fp32 (...), contiguous on this engine's device.  -> ActorGrads.
        ValueError for another tensor or agent, before set_actor(agent), and for a dent that is not finite."""
        t, who = self.torch, "actor_backward"
        a = A.agent_slot(who, agent)
        offset, stride, rows, shape = A.actor_rows(who, obs, a, per_agent, self.device)
        lead = shape[:-1]
        act_offset, act_stride = A.actor_row_values(who, actions, "actions", t.int32, lead, a, self.device)
        A.device_tensor(dlogp, who, "dlogp", t.float32, lead, None, self.device)
        dent = A.finite_float(who, "dent", dent)
        res = ActorGrads(t.empty(L.ACTOR_N_PARAMS, dtype=t.float32, device=self.device), t.empty((), dtype=t.float64, device=self.device))
        self._behind_torch_stream()
        self._call(self.lib.sdc_actor_backward, a, C.c_void_p(obs.data_ptr() + 4 * offset), stride, rows,
                   C.c_void_p(actions.data_ptr() + 4 * act_offset), act_stride, _p(dlogp), dent, _p(res.flat), _p(res.sq_norm),
                   self._stream(), refuses=True, wrote=(obs, actions, dlogp, res.flat, res.sq_norm))
        return res

    def actor_grads(self, batch, agent: int, clip_param: float = 0.2, entropy_coef: float = 0.01, factor=None, old_log_probs=None):
        """The gradient of the reference's actor loss (happo.py update: policy_loss - entropy_coef * dist_entropy, every active mask
        one) for one agent of an OnPolicyBatch with the actor NOW set: evaluate_actions -> ppo_terms -> ppo_dlogp -> actor_backward
        with batch.normalized_advantages(), scale = 1 / (T N) and dent = -entropy_coef / (T N); `factor` and `old_log_probs` as
        actor_update_terms'.  -> (ActorGrads, PPOTerms).  The optimiser step: actor_adam_step on the device (actor_update chains
        the two), or a caller's own over the 6391 values (assign_to) and set_actor."""
        a = A.agent_slot("actor_grads", agent)
        T = batch.n_steps
        n = T * self.n_envs
        obs = batch.obs[:T]
        _, logp, ent = self.evaluate_actions(obs, batch.actions, agents=(a,))
        old = batch.action_log_probs if old_log_probs is None else old_log_probs
        adv = batch.normalized_advantages()
        terms = self.ppo_terms(a, logp, old, adv, clip_param, factor=factor, entropy=ent)
        dlogp = self.ppo_dlogp(a, logp, old, adv, clip_param, factor=factor, scale=1.0 / n)
        return self.actor_backward(a, obs, batch.actions, dlogp, dent=-float(entropy_coef) / n, per_agent=True), terms

    # ------------------------------------------------------------------ the critic's gradient
    def critic_raw_values(self, share_obs):
        """The critic's OWN output for every row of `share_obs` (as critic_values takes it), before `* scale + shift` -- what the
        reference's critic(cent_obs) returns under a ValueNorm (sdc_critic_evaluate: one launch, stream-ordered).  critic_values of
        the same rows is raw * scale + shift in fp32, to the bit.  -> fp32 [...].  ValueError as critic_values'."""
        t = self.torch
        lead = A.share_rows("critic_raw_values", share_obs, self.device)
        raw = t.empty(lead, dtype=t.float32, device=self.device)
        self._behind_torch_stream()
        self._call(self.lib.sdc_critic_evaluate, _p(share_obs), raw.numel(), _p(raw), self._stream(), refuses=True, wrote=(share_obs, raw))
        return raw

    def value_loss(self, raw_values, value_preds, returns, clip_param: float = 0.2, huber_delta: float = 10.0, use_huber_loss: bool = True,
                   use_clipped_value_loss: bool = True, value_norm=None, coef=None, want_loss: bool = True) -> ValueLossTerms:
        """The reference's value loss (v_critic.py cal_value_loss) per element and its derivative per raw value (sdc_value_loss:
        elementwise in fp64, each result rounded once; fixed-order fp64 statistics; stream-ordered): `raw_values` (critic_raw_values'),
        `value_preds` (the stored normalised predictions, OnPolicyBatch.value_preds[:T]) and `returns`, contiguous fp32 tensors of one
        shape on this engine's device.  The target is (returns - shift) / scale: `value_norm` None -- the scale and shift of the critic
        in force (1 and 0 before set_critic; with a ValueNorm installed by set_value_norm the kernel reads them on the device,
        sdc_value_loss_normed, and the host never does) --, a (mean, var) pair, or a ValueNorm, as `critic_params` takes it.  `coef`: dvalue =
        coef * d loss / d raw; None: 1 / n, the reference's mean at value_loss_coef 1.  -> ValueLossTerms.  ValueError for another
        tensor and for what the library refuses (clip_param < 0, huber_delta <= 0 under use_huber_loss, a coef that is not finite)."""
        t, who = self.torch, "value_loss"
        shape = A.any_shape(who, raw_values, "raw_values", t.float32, self.device)
        A.device_tensor(value_preds, who, "value_preds", t.float32, shape, None, self.device)
        A.device_tensor(returns, who, "returns", t.float32, shape, None, self.device)
        n = raw_values.numel()
        coef = 1.0 / max(n, 1) if coef is None else A.finite_float(who, "coef", coef)
        flags = (L.VALUE_LOSS_HUBER if use_huber_loss else 0) | (L.VALUE_LOSS_CLIPPED if use_clipped_value_loss else 0)
        new = lambda: t.empty(shape, dtype=t.float32, device=self.device)
        res = ValueLossTerms(new() if want_loss else None, new(), t.empty(L.PPO_STATS, dtype=t.float64, device=self.device))
        tail = (A.finite_float(who, "clip_param", clip_param), A.finite_float(who, "huber_delta", huber_delta), flags, coef, _p(res.loss),
                _p(res.dvalue), _p(res.stats), self._stream())
        wrote = (raw_values, value_preds, returns, res.loss, res.dvalue, res.stats)
        self._behind_torch_stream()
        if value_norm is None and self._value_norm_installed:
            # (the installed ValueNorm's scale and shift are the device's: the kernel reads them, the host never does)
            self._call(self.lib.sdc_value_loss_normed, n, _p(raw_values), _p(value_preds), _p(returns), *tail, refuses=True, wrote=wrote)
            return res
        if value_norm is None:
            scale, shift = (1.0, 0.0) if self._critic is None else (float(self._critic.scale), float(self._critic.shift))
        else:
            scale, shift = value_norm_scale_shift(value_norm)
        self._call(self.lib.sdc_value_loss, n, _p(raw_values), _p(value_preds), _p(returns), scale, shift, *tail, refuses=True, wrote=wrote)
        return res

    def critic_backward(self, share_obs, dvalue) -> CriticGrads:
        """The gradient of L = sum_r dvalue[r] * raw_r with respect to every parameter of the critic last given to set_critic, over
        stored rows (sdc_critic_backward: the forward recomputed per 16-row tile, the backward on the matrix cores, fixed summation
        order: the same call gives the same bits; stream-ordered).  `share_obs` as critic_values takes it, `dvalue` fp32 of the rows'
        shape (...), contiguous on this engine's device (ValueLossTerms.dvalue).  -> CriticGrads.  ValueError for another tensor and
        before set_critic."""
        t, who = self.torch, "critic_backward"
        lead = A.share_rows(who, share_obs, self.device)
        A.device_tensor(dvalue, who, "dvalue", t.float32, lead, None, self.device)
        res = CriticGrads(t.empty(L.CRITIC_N_PARAMS, dtype=t.float32, device=self.device), t.empty((), dtype=t.float64, device=self.device))
        self._behind_torch_stream()
        self._call(self.lib.sdc_critic_backward, _p(share_obs), dvalue.numel(), _p(dvalue), _p(res.flat), _p(res.sq_norm), self._stream(),
                   refuses=True, wrote=(share_obs, dvalue, res.flat, res.sq_norm))
        return res

    def critic_grads(self, batch, clip_param: float = 0.2, huber_delta: float = 10.0, use_huber_loss: bool = True,
                     use_clipped_value_loss: bool = True, value_loss_coef: float = 1.0, value_norm=None):
        """The gradient of the reference's critic loss (v_critic.py update: value_loss * value_loss_coef, the mean over the batch) for
        an OnPolicyBatch with the critic NOW set: critic_raw_values over batch.share_obs[:T] -> value_loss against
        batch.value_preds[:T] and batch.returns with coef = value_loss_coef / (T N) -> critic_backward.  `value_norm` as value_loss'
        (a caller that keeps a ValueNorm updates it with the returns first, as the reference does, and passes it here).
        -> (CriticGrads, ValueLossTerms).  The optimiser step: critic_adam_step on the device (critic_update chains the two), or a
        caller's own over the 6459 values (assign_to) and set_critic."""
        T = batch.n_steps
        share = batch.share_obs[:T]
        raw = self.critic_raw_values(share)
        coef = A.finite_float("critic_grads", "value_loss_coef", value_loss_coef) / raw.numel()
        terms = self.value_loss(raw, batch.value_preds[:T], batch.returns, clip_param, huber_delta, use_huber_loss, use_clipped_value_loss,
                                value_norm=value_norm, coef=coef)
        return self.critic_backward(share, terms.dvalue), terms

    # ------------------------------------------------------------------ the optimiser step: Adam with clipping, on the device
    def _host_actors(self) -> dict:
        """{slot: SdcActorParams} as the device holds them NOW: the slots stepped since they were set are read back (sdc_get_actor,
        which waits for the device)"""
        for slot in sorted(self._stale_actors):
            p = L.SdcActorParams()
            self._call(self.lib.sdc_get_actor, slot, C.byref(p), refuses=True)
            self._actors[slot] = p
        self._stale_actors.clear()
        return self._actors

    def _host_critic(self):
        """the critic's SdcCriticParams as the device holds it NOW (None before set_critic): read back after a step (sdc_get_critic)"""
        if self._stale_critic:
            p = L.SdcCriticParams()
            self._call(self.lib.sdc_get_critic, C.byref(p), refuses=True)
            self._critic = p
            self._stale_critic = False
        return self._critic

    def _adam_step(self, who, fn, lead, grads, n, lr, betas, eps, weight_decay, max_grad_norm):
        adam = A.adam_struct(who, lr, betas, eps, weight_decay, max_grad_norm)
        flat = A.flat_grads(who, grads, n, self.device)
        norm = self.torch.empty((), dtype=self.torch.float64, device=self.device)
        self._behind_torch_stream()
        self._call(fn, *lead, _p(flat), C.byref(adam), _p(norm), self._stream(), refuses=True, wrote=(flat, norm))
        return norm

    def actor_adam_step(self, agent: int, grads, lr, betas=(0.9, 0.999), eps: float = 1e-5, weight_decay: float = 0.0, max_grad_norm=None):
        """One Adam step with gradient-norm clipping over agent `agent`'s actor ON THE DEVICE (sdc_actor_adam_step: two launches,
        stream-ordered, no synchronisation; include/sustaindc_hip.h THE OPTIMISER STEP states the arithmetic): the parameters the
        engine keeps since set_actor move, and every packed copy the kernels read is rewritten -- launches behind this call on the
        stream see the new actor.  `grads`: an ActorGrads or a flat fp32 tensor [6391] on this engine's device, UNCLIPPED; `eps`
        defaults to the reference's opti_eps; `max_grad_norm` None: no clipping.  A gradient that is not finite changes nothing but
        the state's `skipped` (optim_state).  -> the norm before clipping, fp64 0-dim on the device.  ValueError for another tensor
        or agent, before set_actor(agent), and for what the library refuses about the hyper-parameters."""
        a = A.agent_slot("actor_adam_step", agent)
        norm = self._adam_step("actor_adam_step", self.lib.sdc_actor_adam_step, (a,), grads, L.ACTOR_N_PARAMS, lr, betas, eps, weight_decay,
                               max_grad_norm)
        self._stale_actors.add(a)
        return norm

    def critic_adam_step(self, grads, lr, betas=(0.9, 0.999), eps: float = 1e-5, weight_decay: float = 0.0, max_grad_norm=None):
        """actor_adam_step for the critic (sdc_critic_adam_step): `grads` a CriticGrads or a flat fp32 tensor [6459]; scale and shift
        are no parameters and stay.  -> the norm before clipping, fp64 0-dim on the device."""
        norm = self._adam_step("critic_adam_step", self.lib.sdc_critic_adam_step, (), grads, L.CRITIC_N_PARAMS, lr, betas, eps, weight_decay,
                               max_grad_norm)
        self._stale_critic = True
        return norm

    def actor_update(self, batch, agent: int, clip_param: float = 0.2, entropy_coef: float = 0.01, factor=None, old_log_probs=None, *,
                     lr, betas=(0.9, 0.999), eps: float = 1e-5, weight_decay: float = 0.0, max_grad_norm=None):
        """One whole update of an agent's actor on the device: actor_grads (evaluate, terms, derivative, backward) and actor_adam_step
        behind it, nothing synchronised in between.  -> (PPOTerms, the gradient's norm before clipping)."""
        grads, terms = self.actor_grads(batch, agent, clip_param, entropy_coef, factor=factor, old_log_probs=old_log_probs)
        return terms, self.actor_adam_step(agent, grads, lr, betas, eps, weight_decay, max_grad_norm)

    def critic_update(self, batch, clip_param: float = 0.2, huber_delta: float = 10.0, use_huber_loss: bool = True,
                      use_clipped_value_loss: bool = True, value_loss_coef: float = 1.0, value_norm=None, *, lr, betas=(0.9, 0.999),
                      eps: float = 1e-5, weight_decay: float = 0.0, max_grad_norm=None):
        """One whole update of the critic on the device: critic_grads and critic_adam_step behind it, nothing synchronised in between.
        -> (ValueLossTerms, the gradient's norm before clipping)."""
        grads, terms = self.critic_grads(batch, clip_param, huber_delta, use_huber_loss, use_clipped_value_loss, value_loss_coef, value_norm)
        return terms, self.critic_adam_step(grads, lr, betas, eps, weight_decay, max_grad_norm)

    def actor_state_dict(self, agent: int) -> dict:
        """Agent `agent`'s actor as the device holds it now, under the reference's StochasticPolicy state_dict keys (host tensors;
        without base.feature_norm.* when the feature LayerNorm is off).  It waits for the device.  ValueError before set_actor."""
        a = A.agent_slot("actor_state_dict", agent)
        if a not in self._actors:
            raise ValueError(f"actor_state_dict: no actor is set for agent {a} (set_actor first)")
        p = self._host_actors()[a]
        return _struct_state_dict(p, _ACTOR_SHAPES, _ACTOR_SD_KEYS, {}, bool(p.use_feature_normalization))

    def critic_state_dict(self) -> dict:
        """The critic as the device holds it now, under the reference's VNet state_dict keys (v_out.weight [1, 64], v_out.bias [1]).
        It waits for the device.  ValueError before set_critic."""
        if self._critic is None:
            raise ValueError("critic_state_dict: set_critic first")
        p = self._host_critic()
        return _struct_state_dict(p, _CRITIC_SHAPES, _CRITIC_SD_KEYS, {"w3": (1, 64), "b3": (1,)}, bool(p.flags & 1))

    def optim_state(self, which) -> dict:
        """The optimiser state of agent slot `which` (0 .. 2) or of "critic", for a checkpoint: {m, v: fp32 host arrays in the
        gradient's order, step, beta1_pow, beta2_pow, skipped} -- and for "critic" with a ValueNorm installed (set_value_norm) also
        value_norm: its three running values, training state as the moments are.  It waits for the device.  ValueError before the
        network is set."""
        slot = A.optim_which("optim_state", which)
        n = L.CRITIC_N_PARAMS if slot is None else L.ACTOR_N_PARAMS
        m, v, st = np.empty(n, np.float32), np.empty(n, np.float32), L.SdcOptimState()
        ptrs = (C.c_void_p(m.ctypes.data), C.c_void_p(v.ctypes.data), C.byref(st))
        if slot is None:
            self._call(self.lib.sdc_get_critic_optim, *ptrs, refuses=True)
        else:
            self._call(self.lib.sdc_get_actor_optim, slot, *ptrs, refuses=True)
        out = dict(m=m, v=v, step=int(st.step), beta1_pow=float(st.beta1_pow), beta2_pow=float(st.beta2_pow), skipped=int(st.skipped))
        if slot is None and self._value_norm_installed:      # (the critic's running ValueNorm is training state as the moments are)
            vn = self.value_norm_state()
            out["value_norm"] = {k: vn[k] for k in ("running_mean", "running_mean_sq", "debiasing_term")}
        return out

    def load_optim_state(self, which, state: dict):
        """optim_state's dict back into the network `which` (its parameters are set_actor's / set_critic's to give, before this); a
        "value_norm" entry of the critic's is installed with set_value_norm.
        ValueError for a wrong shape and for what the library refuses (step < 0, a power outside (0, 1], a moment not finite)."""
        slot = A.optim_which("load_optim_state", which)
        m, v, st = A.optim_arrays("load_optim_state", state, L.CRITIC_N_PARAMS if slot is None else L.ACTOR_N_PARAMS)
        ptrs = (C.c_void_p(m.ctypes.data), C.c_void_p(v.ctypes.data), C.byref(st))
        if slot is None:
            self._call(self.lib.sdc_set_critic_optim, *ptrs, refuses=True)
            if state.get("value_norm") is not None:      # (optim_state's, of an engine with a ValueNorm installed)
                self.set_value_norm(state["value_norm"])
        else:
            self._call(self.lib.sdc_set_actor_optim, slot, *ptrs, refuses=True)

    def set_critic_value_norm(self, value_norm):
        """The critic's ValueNorm alone (sdc_set_critic_norm: stream-ordered, the parameters stay on the device): `value_norm` as
        critic_params takes it -- None, a (mean, var) pair or a ValueNorm.  critic_values, collect's value_preds and value_loss'
        default target follow from the next launch on.  ValueError before set_critic and for a scale that is not positive."""
        scale, shift = value_norm_scale_shift(value_norm)
        self._call(self.lib.sdc_set_critic_norm, float(scale), float(shift), self._stream(), refuses=True)
        self._critic.scale, self._critic.shift = float(scale), float(shift)      # (no parameters: the host copy follows at once)
        self._value_norm_installed = False      # (the library uninstalls: scale and shift were set by hand)

    # ------------------------------------------------------------------ train on the device: ValueNorm, shuffled mini-batches, happo_train
    def set_value_norm(self, value_norm):
        """A ValueNorm KEPT ON THE DEVICE (sdc_set_value_norm): `value_norm` as `critic_params` takes it -- a ValueNorm object or dict
        with running_mean, running_mean_sq and debiasing_term; a (mean, var) pair becomes (mean, var + mean^2, 1) -- or None, which
        uninstalls (the critic keeps the scale and shift it has).  While one is installed the critic's scale and shift follow it:
        value_norm_update moves them on the device, and value_loss / critic_grads / critic_update called with value_norm=None read them
        there.  set_critic and set_critic_value_norm uninstall.  The call waits for the device.  ValueError before set_critic and for
        values that are not finite."""
        st = A.value_norm_struct("set_value_norm", value_norm)
        self._call(self.lib.sdc_set_value_norm, None if st is None else C.byref(st), refuses=True)
        self._value_norm_installed = st is not None
        self._stale_critic = True      # (scale and shift of the host copy)
        if st is None:
            self._host_critic()

    def value_norm_state(self) -> dict:
        """The installed ValueNorm as the device holds it now: {running_mean, running_mean_sq, debiasing_term, scale, shift} as Python
        floats of the fp32 values (the first three are what set_value_norm takes).  It waits for the device.  ValueError while none is
        installed."""
        st = L.SdcValueNorm()
        self._call(self.lib.sdc_get_value_norm, C.byref(st), refuses=True)
        self._stale_critic = True
        p = self._host_critic()
        return dict(running_mean=float(st.running_mean), running_mean_sq=float(st.running_mean_sq), debiasing_term=float(st.debiasing_term),
                    scale=float(p.scale), shift=float(p.shift))

    def value_norm_update(self, returns, beta: float = 0.99999):
        """ValueNorm.update(returns) for the installed ValueNorm, on the device (sdc_value_norm_update: two launches, stream-ordered,
        fixed-order fp64 sums, the reference's fp32 recurrence; include/sustaindc_hip.h states it): `returns` a contiguous fp32 tensor
        of any shape on this engine's device.  The critic's scale and shift follow: launches behind this call see the new statistics.
        ValueError while no ValueNorm is installed, for an empty tensor and for beta outside [0, 1)."""
        t, who = self.torch, "value_norm_update"
        A.any_shape(who, returns, "returns", t.float32, self.device)
        self._behind_torch_stream()
        self._call(self.lib.sdc_value_norm_update, _p(returns), returns.numel(), A.finite_float(who, "beta", beta), self._stream(),
                   refuses=True, wrote=(returns,))
        self._stale_critic = True      # (scale and shift of the host copy)

    def permutation(self, n: int, seed: int, stream_id: int = 0):
        """A keyed pseudo-random bijection of 0 .. n-1 as an int32 tensor [n] on this engine's device (sdc_permutation: one launch, one
        lane per output, no sort; stream-ordered).  The same (n, seed, stream_id) give the same bits on every run; it shuffles rows, it
        is no uniform draw from all n! permutations (include/sustaindc_hip.h).  ValueError for n outside 1 .. 2^31 - 1."""
        t = self.torch
        n = int(n)
        if not 1 <= n <= L.PERM_MAX_N:
            raise ValueError(f"permutation: n = {n} outside [1, {L.PERM_MAX_N}]")
        perm = t.empty(n, dtype=t.int32, device=self.device)
        self._call(self.lib.sdc_permutation, n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFFFFFFFFFF, _p(perm), self._stream(),
                   refuses=True, wrote=(perm,))
        return perm

    def minibatch(self, batch, indices, agent=None, critic: bool = True, into=None, *, actors: bool = True, factor=None) -> MiniBatch:
        """The rows `indices` of an OnPolicyBatch as a dense mini-batch (sdc_gather_rows: ONE launch for all fields, stream-ordered):
        `indices` int32 [T' N] on this engine's device, indices into the T N rows of batch.flat() -- a permutation(), a slice of one,
        a torch.randperm cast to int32 -- -> a MiniBatch whose per-step fields are [T', N, ...]; actor_update, actor_update_terms and
        critic_update run on it unchanged.  `agent`: only that agent's column of obs, actions, action_log_probs, logits and entropy is
        written (a third of the bytes); `critic` False: share_obs, values, value_preds and returns are not gathered; `actors` False:
        the per-agent fields and the advantages are not; rewards, masks and dones (uint8: gathered by torch ops) only with both.
        adv_mean / adv_std are the parent's, so normalized_advantages() gives the parent's normalisation.  `factor` fp32 [T, N]: gathered
        alongside into MiniBatch.factor.  `into`: a MiniBatch of an earlier call with the same arguments, whose tensors are written
        again.  An index outside [0, T N) is never an address: that row comes back as zeros and MiniBatch.bad is 1.  ValueError when
        len(indices) is not a positive multiple of N, and for tensors of another kind."""
        t, who, N = self.torch, "minibatch", self.n_envs
        a = None if agent is None else A.agent_slot(who, agent)
        if not isinstance(batch, OnPolicyBatch):
            raise ValueError(f"{who}: batch must be an OnPolicyBatch")
        if not (actors or critic):
            raise ValueError(f"{who}: neither the actors' nor the critic's fields are asked for")
        T = batch.n_steps
        A.device_tensor(indices, who, "indices", t.int32, (A.SOME,), "(rows,)", self.device)
        rows = indices.numel()
        if rows % N:
            raise ValueError(f"{who}: len(indices) = {rows} is not a positive multiple of n_envs = {N}")
        Tm = rows // N
        plan = A.minibatch_segments(a, actors, critic)
        if len(plan) + (factor is not None) > L.GATHER_MAX_SEGMENTS:
            raise ValueError(f"{who}: more than {L.GATHER_MAX_SEGMENTS} arrays in one gather")
        book = actors and critic
        names = [name for name, _, _, _ in plan] + (["dones"] if book else [])
        if into is None:
            fields = dict.fromkeys(OnPolicyBatch.FIELDS)
            for name in names:
                src = getattr(batch, name)
                fields[name] = t.empty((Tm, N) + tuple(src.shape[2:]), dtype=src.dtype, device=self.device)
            into = MiniBatch(Tm, None if factor is None else t.empty((Tm, N), dtype=t.float32, device=self.device),
                             t.zeros(1, dtype=t.int32, device=self.device), **fields)
        else:
            if not isinstance(into, MiniBatch) or into.n_steps != Tm or (factor is None) != (into.factor is None):
                raise ValueError(f"{who}: into must be a MiniBatch of {Tm} steps from a call with the same arguments")
            into.bad.zero_()
        into.adv_mean, into.adv_std, into.last_done = batch.adv_mean, batch.adv_std, batch.last_done
        segs = (L.SdcGatherSegment * (len(plan) + (factor is not None)))()
        used = [indices, into.bad]
        pairs = [(getattr(batch, name), getattr(into, name), off, n, row, name) for name, off, n, row in plan]
        if factor is not None:
            A.device_tensor(factor, who, "factor", t.float32, (T, N), "(T, n_envs)", self.device)
            pairs.append((factor, into.factor, 0, 1, 1, "factor"))
        for g, (src, dst, off, n, row, name) in zip(segs, pairs):
            if src is None or dst is None:
                raise ValueError(f"{who}: the batch or `into` holds no {name}")
            want = (Tm, N) + tuple(src.shape[2:])
            if not (src.is_contiguous() and dst.is_contiguous() and src.shape[0] >= T and tuple(dst.shape) == want and dst.dtype == src.dtype
                    and src.element_size() == 4 and src.device == self.device and dst.device == self.device):
                raise ValueError(f"{who}: {name} must be contiguous 4-byte tensors on {self.device}, `into`'s of shape {want}")
            g.src, g.dst = src.data_ptr() + 4 * off, dst.data_ptr() + 4 * off
            g.src_stride = g.dst_stride = row
            g.n_dwords = n
            used += [src, dst]
        self._behind_torch_stream()
        self._call(self.lib.sdc_gather_rows, _p(indices), rows, T * N, segs, len(segs), _p(into.bad), self._stream(), refuses=True, wrote=used)
        if book:      # (uint8 rows are no dword rows: torch gathers them, an index outside the rows giving 0 as above)
            ok = (indices >= 0) & (indices < T * N)
            picked = batch.dones[:T].reshape(-1).index_select(0, indices.clamp(0, T * N - 1).long())
            into.dones.copy_((picked * ok).view(Tm, N))
        return into

    def happo_train(self, batch, *, seed=None, ppo_epoch: int = 5, critic_epoch: int = 5, actor_num_mini_batch: int = 1,
                    critic_num_mini_batch: int = 1, agent_order=(0, 1, 2), use_factor: bool = True, indices=None, clip_param: float = 0.2,
                    entropy_coef: float = 0.01, huber_delta: float = 10.0, use_huber_loss: bool = True, use_clipped_value_loss: bool = True,
                    value_loss_coef: float = 1.0, lr, critic_lr=None, betas=(0.9, 0.999), eps: float = 1e-5, weight_decay: float = 0.0,
                    max_grad_norm=None, update_value_norm: bool = True, beta: float = 0.99999) -> TrainInfo:
        """The reference's OnPolicyHARunner.train() over one OnPolicyBatch, on the device, nothing read by the host.  For every agent
        of `agent_order`: its log-probabilities over the whole batch before the update (evaluate_actions); `ppo_epoch` epochs, each
        over one permutation of the T N rows -- permutation(T N, seed, (agent << 32) | epoch) -- cut into `actor_num_mini_batch` pieces
        of (T / num) N rows, each piece gathered (minibatch, the agent's columns and the factor) and given to actor_update; then the
        HAPPO factor is multiplied by exp(new - old) over the whole batch (actor_update_terms).  The critic follows: `critic_epoch`
        epochs over permutation(T N, seed, (3 << 32) | epoch) cut into `critic_num_mini_batch` pieces; per piece value_norm_update on
        the piece's returns first -- while a ValueNorm is installed (set_value_norm) and `update_value_norm` is on -- then
        critic_update.  `indices`: {(who, epoch): int32 [T N] on the device}, who an agent slot or "critic": these replace the draws
        (a test replays the reference's own permutations); `seed` may be None when it names every epoch.  The loss arguments are
        actor_update's and critic_update's, `lr` the actors' and `critic_lr` the critic's (None: lr), the Adam arguments both's.
        -> TrainInfo.  ValueError when a num_mini_batch does not divide T (the reference drops the remainder; we refuse)."""
        who, N, T = "happo_train", self.n_envs, batch.n_steps
        order = A.agent_slots(who, agent_order)
        a_rows = A.minibatch_rows(who, T, N, actor_num_mini_batch)
        c_rows = A.minibatch_rows(who, T, N, critic_num_mini_batch)
        indices = {} if indices is None else indices

        def draw(key, stream_who, epoch):
            if key in indices:
                A.device_tensor(indices[key], who, f"indices[{key!r}]", self.torch.int32, (T * N,), f"({T * N},)", self.device)
                return indices[key]
            if seed is None:
                raise ValueError(f"{who}: no seed and no indices for {key!r}")
            return self.permutation(T * N, seed, A.perm_stream_id(stream_who, epoch))

        adam = dict(betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        info, factor, mb = TrainInfo(), None, None
        for a in order:
            _, old_lp, _ = self.evaluate_actions(batch.obs[:T], batch.actions, agents=(a,), want_entropy=False)
            ups = info.actor[a] = []
            for e in range(int(ppo_epoch)):
                perm = draw((a, e), a, e)
                for k in range(0, T * N, a_rows):
                    mb = self.minibatch(batch, perm[k:k + a_rows], agent=a, critic=False, into=mb, factor=factor)
                    terms, norm = self.actor_update(mb, a, clip_param, entropy_coef, factor=mb.factor, lr=lr, **adam)
                    ups.append((terms.stats, norm))
            if use_factor:
                new_factor = self.actor_update_terms(batch, a, clip_param, factor=factor, old_log_probs=old_lp).factor
                if factor is None:
                    mb = None      # (the next agent's pieces carry a factor: other tensors)
                factor = new_factor
        info.factor = factor
        mb = None
        vn = update_value_norm and self._value_norm_installed
        for e in range(int(critic_epoch)):
            perm = draw(("critic", e), 3, e)
            for k in range(0, T * N, c_rows):
                mb = self.minibatch(batch, perm[k:k + c_rows], actors=False, into=mb)
                if vn:
                    self.value_norm_update(mb.returns, beta)
                terms, norm = self.critic_update(mb, clip_param, huber_delta, use_huber_loss, use_clipped_value_loss, value_loss_coef,
                                                 lr=lr if critic_lr is None else critic_lr, **adam)
                info.critic.append((terms.stats, norm))
        return info

    # ------------------------------------------------------------------ state access (parity injection / checkpoint)
    def _state_array(self, name):
        return A.state_array(name, self._sizes)

    def get_state(self, name: str) -> np.ndarray:
        a = self._state_array(name)
        self._call(self.lib.sdc_get_state, name.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes)
        return a

    def set_state(self, name: str, value):
        a = self._state_array(name)
        if (isinstance(value, np.ndarray) and value.dtype == a.dtype and value.shape == a.shape and
                value.flags.c_contiguous):
            a = value       # already in the library's layout: no host copy (a batch's rings are GBs)
        else:
            a[...] = value
        self._call(self.lib.sdc_set_state, name.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes)

    def state_dict(self) -> dict:
        """Full env checkpoint (the reference never checkpoints env state): the arrays the kernels own
        and "meta" -- the library's state layout (sdc_state_layout), the engine's configuration and the current RNG seed, which
        keys every future reset."""
        sd = {n: self.get_state(n) for n in _CHECKPOINT}
        sd["meta"] = dict(self._identity(), seed=self.seed)
        return sd

    def load_state_dict(self, sd: dict):
        """Restore a state_dict().  Refused with a ValueError naming the key: a dict without "meta", or one whose state layout,
        n_envs, episode_steps, hist_cap, queue_max_len, max_roll_days, n_locations, n_dc_configs or env_index_base differs
        from this engine's.  The saved seed is applied.  Trace tables, DC parameters and the rest of the constructor's
        arguments are configuration, not state: the engine keeps its own (set them as for the engine that saved the dict)."""
        meta = sd.get("meta")
        if not isinstance(meta, dict):
            raise ValueError("load_state_dict: the checkpoint has no 'meta' entry (saved by an older build?)")
        mine = self._identity()
        for k in _META_MUST_MATCH:
            if k not in meta or meta[k] != mine[k]:
                raise ValueError(f"load_state_dict: checkpoint {k} = {meta.get(k)!r}, this engine's is {mine[k]!r}")
        if "seed" not in meta:
            raise ValueError("load_state_dict: checkpoint has no seed")
        for n, v in sd.items():
            if n != "meta":
                self.set_state(n, v)
        self.set_seed(meta["seed"])

    def clone_envs(self, src, dst):
        """Env dst[k] becomes an exact copy of env src[k] (copy.deepcopy of the reference's SustainDC, for envs of this batch), on
        the device, ordered after the work already queued like a step (sdc_clone_envs).  src / dst: int sequences or arrays of the
        same length; a scalar src is broadcast.  The engine's obs / share_obs rows follow, so eng.obs[dst] == eng.obs[src]
        afterwards; the rest of the state is the library's.  dst finishes src's current episode exactly; its reset draws stay keyed
        on its own index (env_index_base + dst), so from its next reset on it runs episodes of its own.  A lock-step batch stays on
        the specialised kernels when every src is at the same episode step.  ValueError for what the library refuses: an empty
        dst, an index outside [0, n_envs), a repeated dst, a dst that is also a src, no reset() yet.  -> (obs, share_obs) views."""
        s, d = self.clone_pairs(src, dst)
        self._call(self.lib.sdc_clone_envs, _ip(s), _ip(d), int(d.shape[0]), *self._obs_ptrs, self._stream(), refuses=True)
        return self.obs, self.share_obs

    def clone_pairs(self, src, dst):
        """clone_envs' arguments as two int32 arrays of one length (a scalar src broadcast); ValueError for a malformed pair list
        (the library checks the rest)."""
        return A.clone_pairs(src, dst, self.n_envs)

    def snapshot(self, envs=None) -> EnvSnapshot:
        """The complete state of envs (default: all) in a device buffer of their own (sdc_snapshot_envs), ordered after the work already
        queued like a step, without a device synchronisation.  Read-only on the engine: taking snapshots does not change the run.  The
        rows can be restored into any envs of this engine or of another with the same state layout, episode_steps, hist_cap,
        queue_max_len, max_roll_days, locations and dc configs (`restore`), on another GPU after `.to(device)`.  ValueError for what the
        library refuses: no env, an index outside [0, n_envs), more envs than the batch, no reset() yet."""
        t = self.torch
        e = self._all_envs.copy() if envs is None else A.int_ids(envs, "snapshot: envs").reshape(-1)
        n = int(e.shape[0])
        manifest = np.zeros((max(n, 1), L.SNAPSHOT_MANIFEST), dtype=np.int32)
        rows = t.empty((n, int(self.lib.sdc_snapshot_row_bytes(self._h))), dtype=t.uint8, device=self.device)
        self._call(self.lib.sdc_snapshot_envs, _ip(e), n, _p(rows), _ip(manifest), *self._obs_ptrs, self._stream(),
                   refuses=True, wrote=(rows,))
        mine = self._identity()
        return EnvSnapshot(rows, manifest[:n], {k: mine[k] for k in _SNAPSHOT_MUST_MATCH}, e)

    def restore_pairs(self, snap: EnvSnapshot, envs=None, rows=None):
        """restore's arguments as (rows, envs), two int32 arrays of one length: envs default to snap.envs, rows to 0 .. len(snap) - 1 (a
        scalar broadcast); ValueError for a malformed list (the library checks the rest)."""
        return A.restore_pairs(snap.envs, envs, rows)

    def restore(self, snap: EnvSnapshot, envs=None, rows=None):
        """Env envs[k] becomes snapshot row rows[k] (sdc_restore_envs): by default row k goes back into env snap.envs[k]; a scalar
        `rows` is broadcast (one state into several envs).  One launch ordered like a step, no device synchronisation; the engine's
        obs / share_obs rows follow.  A restore that leaves the batch in lock-step (a whole-batch rewind) keeps the specialised
        kernels.  A restored env finishes the saved episode exactly; its later episodes are keyed on its own global index and this
        engine's seed.  ValueError for a snapshot of another state layout or configuration, rows on another device, and what the
        library refuses (an index out of range, a repeated env, no reset() yet).  -> (obs, share_obs) views."""
        t = self.torch
        mine = self._identity()
        for k in _SNAPSHOT_MUST_MATCH:
            if snap.meta.get(k) != mine[k]:
                raise ValueError(f"restore: snapshot {k} = {snap.meta.get(k)!r}, this engine's is {mine[k]!r}")
        if snap.rows.device != self.device:
            raise ValueError(f"restore: the snapshot's rows are on {snap.rows.device}, this engine runs on {self.device} "
                             "(snapshot.to(device))")
        rb = int(self.lib.sdc_snapshot_row_bytes(self._h))
        if snap.rows.dtype != t.uint8 or snap.rows.dim() != 2 or snap.rows.shape[1] != rb or not snap.rows.is_contiguous():
            raise ValueError(f"restore: rows must be a contiguous uint8 tensor [n, {rb}], got {tuple(snap.rows.shape)}")
        m = np.ascontiguousarray(snap.manifest, dtype=np.int32)
        if m.shape != (snap.rows.shape[0], L.SNAPSHOT_MANIFEST):
            raise ValueError(f"restore: manifest of shape {m.shape} for {snap.rows.shape[0]} rows")
        r, d = self.restore_pairs(snap, envs, rows)
        self._call(self.lib.sdc_restore_envs, _ip(r), _ip(d), int(d.shape[0]), _p(snap.rows), int(snap.rows.shape[0]), _ip(m),
                   *self._obs_ptrs, self._stream(), refuses=True, wrote=(snap.rows,))
        return self.obs, self.share_obs

    # ------------------------------------------------------------------ mark / rewind / lookahead
    def mark(self, envs=None, max_steps: int = 16) -> EnvMark:
        """Save what the next `max_steps` steps can change in envs (default: the whole batch) into a device buffer (sdc_mark_envs): one
        launch ordered like a step, no device synchronisation, read-only on the engine.  `rewind(mark)` undoes up to max_steps steps
        taken since -- inside one episode, into the same envs of this engine.  One live mark per env: a later mark of an env, its reset
        (auto-reset included), set_state / load_state_dict, a clone or restore INTO it kill the mark.  ValueError for what the library
        refuses: max_steps outside [1, MARK_MAX_STEPS], no env, an index out of range or repeated, no reset() yet."""
        t = self.torch
        K = int(max_steps)
        rb = int(self.lib.sdc_mark_row_bytes(K))
        if rb == 0:
            raise ValueError(f"mark: max_steps = {K} outside [1, {L.MARK_MAX_STEPS}]")
        whole = envs is None
        e = self._all_envs if whole else A.int_ids(envs, "mark: envs").reshape(-1)
        n = int(e.shape[0])
        manifest = np.empty((max(n, 1), L.MARK_MANIFEST), dtype=np.int32)
        rows = t.empty((n, rb), dtype=t.uint8, device=self.device)
        self._call(self.lib.sdc_mark_envs, None if whole else _ip(e), n, K, _p(rows), _ip(manifest), *self._obs_ptrs, self._stream(),
                   refuses=True, wrote=(rows,))
        return EnvMark(rows, manifest[:n], e, K, whole)

    def rewind(self, mark: EnvMark, envs=None):
        """Undo the steps taken since `mark` in its envs (default), or in a subset of them (sdc_rewind_envs): one launch ordered like a
        step, no device synchronisation; the engine's obs / share_obs rows (and the closed loop's copy) follow.  A whole-batch rewind
        of a lock-step batch stays on the kernel it was on; a rewind of some envs leaves the batch out of lock-step, as a masked reset
        does.  The mark stays alive: it may be rewound to again.  ValueError, with the engine untouched, for a mark of another engine,
        a dead mark (see `mark`), an env that is not in the mark, and more than max_steps steps taken since the mark -- after which
        the mark is dead for good.  -> (obs, share_obs) views."""
        t = self.torch
        if not isinstance(mark, EnvMark):
            raise ValueError("rewind: not an EnvMark")
        if mark.rows.device != self.device:
            raise ValueError(f"rewind: the mark's rows are on {mark.rows.device}, this engine runs on {self.device}")
        if envs is None:
            e, rows, m, whole = mark.envs, mark.rows, mark.manifest, mark.whole
        else:       # some of the mark's envs: their rows gathered into a buffer of their own (row k belongs to envs[k])
            e = np.ascontiguousarray(A.int_ids(envs, "rewind: envs").reshape(-1))
            pos = mark.positions(e)
            rows = mark.rows[t.as_tensor(pos, device=self.device)].contiguous() if pos.size else mark.rows[:0]
            m, whole = np.ascontiguousarray(mark.manifest[pos]), False
        n = int(e.shape[0])
        if n == 0:
            raise ValueError("rewind: no env")
        self._call(self.lib.sdc_rewind_envs, None if whole else _ip(e), n, _p(rows), _ip(m), *self._obs_ptrs, self._stream(),
                   refuses=True, wrote=(rows,))
        return self.obs, self.share_obs

    def lookahead(self, actions):
        """Score M candidate action sequences of K steps from the current state and come back to it: `actions` int32 device tensor
        [M, K, N, 3].  The batch is marked (max_steps = K); every candidate is rolled out (`rollout`), its rewards summed over the K
        steps on the device in fp64, in step order, and the batch rewound.  -> returns [M, N, 3] float64 on the device; the engine --
        state, output buffers, closed-loop copy -- is where it was, with one difference: a rewind clears the header's re-centring
        stamps, so deferred re-centrings in flight at the call are dropped and re-requested by the steps that need them (window
        placement and info[reserved] may differ from a run that never looked ahead; no other output does).  The rollouts ask for
        the info rows although they are thrown away: without them the batch is not the specialised kernels' case (csrc/sdc_dispatch.hpp
        sdc_specialised_ok) and every candidate would run the general kernel.  ValueError for a K that would finish an episode:
        K >= steps_to_episode_end() with auto_reset (the reset would kill the mark), K > steps_to_episode_end() without; and for
        K > MARK_MAX_STEPS."""
        t = self.torch
        A.device_tensor(actions, "lookahead", "actions", t.int32, (A.SOME, A.SOME, self.n_envs, 3), "(M, K, n_envs, 3)")
        M, K = int(actions.shape[0]), int(actions.shape[1])
        A.check_horizon("lookahead", K, self.steps_to_episode_end(), self.config["auto_reset"])
        with t.cuda.device(self.device):
            keep, keep_final = self.out_flat.clone(), self.final_obs.clone()     # (the last step's outputs: rollout overwrites them)
            mk = self.mark(max_steps=K)
            returns = t.empty((M, self.n_envs, L.N_AGENTS), dtype=t.float64, device=self.device)
            for c in range(M):
                rew = self.rollout(actions[c])[2]
                acc = returns[c]
                acc.copy_(rew[0])
                for k in range(1, K):
                    acc.add_(rew[k])      # (fp32 -> fp64 is exact; one addition per step, in step order)
                self.rewind(mk)
            self.out_flat.copy_(keep)
            self.final_obs.copy_(keep_final)
        return returns

    def plan(self, actions, reward_weights=(1.0, 1.0, 1.0), gamma: float = 1.0, info_weights=None) -> PlanResult:
        """Score M candidate action sequences of K steps from the current state, pick every env's best, and come back (sdc_plan): one
        library call -- mark, per candidate rollout / score / rewind, select -- with no Python between the launches and no per-step
        output the caller has to hold; what `lookahead` does in a loop, plus the objective and the selection.  `actions` int32 device
        tensor [M, K, N, 3].  A candidate's score is the discounted sum over its steps (gamma ** k, built by repeated multiplication) of
        reward_weights . (r_ls, r_dc, r_bat) + sum of info_weights[key] * info[key] -- `info_weights` a dict of at most PLAN_MAX_COLS
        info key names (dc_rl_amd._lib.INFO_COLS: bat_CO2_footprint, dc_water_usage, ls_tasks_dropped, ...) -> weight; fp64, in step
        order (the exact operation order: include/sustaindc_hip.h).  The best candidate is the lowest-numbered one with the highest
        score.  -> PlanResult(best [N], action [N, 3] = actions[best, 0], score [M, N], returns [M, N, 3]).
        The engine -- state, output buffers, closed-loop copy -- is where it was, with `lookahead`'s one difference (the rewinds clear
        the re-centring stamps) and the same price: the call uses up the envs' one live mark, so a mark taken earlier is dead
        afterwards.  A slot on a built-in policy ignores its action column.  The rollouts read the traces of the steps ahead as the
        episode holds them (perfect foresight) unless a forecast is set: `set_plan_forecast`.  ValueError, with the engine untouched, for malformed
        actions, an unknown info key or too many, and what the library refuses: K > MARK_MAX_STEPS, K >= steps_to_episode_end() with
        auto_reset (> without), no reset() yet, gamma outside (0, 1], verify mode (debug_flags DEBUG_VERIFY: rollouts have none)."""
        t = self.torch
        A.device_tensor(actions, "plan", "actions", t.int32, (A.SOME, A.SOME, self.n_envs, 3), "(M, K, n_envs, 3)", self.device, True)
        M, K, N = int(actions.shape[0]), int(actions.shape[1]), self.n_envs
        A.check_horizon("plan", K)
        obj = plan_objective(reward_weights, gamma, info_weights)
        returns = t.empty((M, N, L.N_AGENTS), dtype=t.float64, device=self.device)
        score = t.empty((M, N), dtype=t.float64, device=self.device)
        best = t.empty((N,), dtype=t.int32, device=self.device)
        action = t.empty((N, 3), dtype=t.int32, device=self.device)
        self._call(self.lib.sdc_plan, M, K, _p(actions), C.byref(obj), _p(returns), _p(score), _p(best), _p(action), *self._obs_ptrs,
                   self._stream(), refuses=True, wrote=(returns, score, best, action, actions))
        return PlanResult(best, action, score, returns)

    def set_plan_terms(self, limits=None, terminal=None):
        """What a linear objective cannot say, kept on the engine (sdc_set_plan_terms): every later `plan`, `plan_cem` and
        `plan_cem_groups` scores with it until it is cleared.  `limits`: a dict info key -> (low, high, weight), `low` / `high` each a
        float or None -- every step the candidate pays weight * max(0, low - info[key]) and weight * max(0, info[key] - high) (each
        side given is one entry, in dict order, low before high; at most PLAN_MAX_LIMITS entries; weight >= 0).  `terminal`: a dict
        info key -> weight of at most PLAN_MAX_TERMINAL keys -- the info row the horizon's LAST step leaves, weighed and discounted as
        one step further (gamma ** K), is added to the score: what a finite horizon otherwise defers for free (ls_tasks_in_queue,
        ls_oldest_task_age, bat_SOC, ...).  No arguments (or two empty dicts) clears the terms.  `returns` never see them; the exact
        operation order: include/sustaindc_hip.h.  Whether a plan keeps a limit shows in its rollout: `lookahead` / `rollout` of the
        chosen sequence gives the info rows.  Host state: nothing is enqueued.  ValueError, with the terms set before still in force,
        for an unknown info key, too many entries, and what the library refuses (a bound or weight that is not finite, a negative
        limit weight)."""
        s = L.SdcPlanTerms()
        entries = []
        for key, spec in dict(limits or {}).items():
            if key not in L.INFO_IDX:
                raise ValueError(f"set_plan_terms: limits key {key!r} is not an info column (dc_rl_amd._lib.INFO_COLS)")
            try:
                low, high, weight = spec
            except (TypeError, ValueError):
                raise ValueError(f"set_plan_terms: limits[{key!r}] must be (low, high, weight)") from None
            entries += [(L.INFO_IDX[key], side, float(b), float(weight)) for side, b in ((-1, low), (1, high)) if b is not None]
        if len(entries) > L.PLAN_MAX_LIMITS:
            raise ValueError(f"set_plan_terms: limits make {len(entries)} entries (one per side given), at most {L.PLAN_MAX_LIMITS} can be set")
        s.n_limits = len(entries)
        for j, (col, side, bound, weight) in enumerate(entries):
            s.limit_col[j], s.limit_side[j], s.limit_bound[j], s.limit_weight[j] = col, side, bound, weight
        term = dict(terminal or {})
        if len(term) > L.PLAN_MAX_TERMINAL:
            raise ValueError(f"set_plan_terms: terminal names {len(term)} keys, at most {L.PLAN_MAX_TERMINAL} can be weighed")
        s.n_terminal = len(term)
        for j, (key, weight) in enumerate(term.items()):
            if key not in L.INFO_IDX:
                raise ValueError(f"set_plan_terms: terminal key {key!r} is not an info column (dc_rl_amd._lib.INFO_COLS)")
            s.terminal_col[j], s.terminal_weight[j] = L.INFO_IDX[key], float(weight)
        self._set_plan_terms_struct(s)

    def _set_plan_terms_struct(self, s: L.SdcPlanTerms):
        self._call(self.lib.sdc_set_plan_terms, C.byref(s), refuses=True)

    def _plan_terms_struct(self) -> L.SdcPlanTerms:
        """the terms as the library holds them (what a copy of this engine is given: SustainDCVecEnv.__deepcopy__)"""
        s = L.SdcPlanTerms()
        self._call(self.lib.sdc_get_plan_terms, C.byref(s), refuses=True)
        return s

    @property
    def plan_terms(self):
        """The terms in force, read back from the library (sdc_get_plan_terms) -> (limits, terminal), the two dicts `set_plan_terms`
        takes (both empty: none set), so that `set_plan_terms(*e.plan_terms)` sets the same entries in the same order.  ValueError for
        terms set through the C ABI that the dicts cannot say: a column with two entries on one side, or with two weights."""
        s = self._plan_terms_struct()
        limits = {}
        for j in range(s.n_limits):
            key, at = L.INFO_COLS[s.limit_col[j]], 0 if s.limit_side[j] < 0 else 1
            had = limits.setdefault(key, [None, None, s.limit_weight[j]])
            if had[at] is not None or had[2] != s.limit_weight[j]:
                raise ValueError(f"plan_terms: the entries on {key!r} do not fit (low, high, weight): read them with sdc_get_plan_terms")
            had[at] = s.limit_bound[j]
        terminal = {}
        for j in range(s.n_terminal):
            key = L.INFO_COLS[s.terminal_col[j]]
            if key in terminal:
                raise ValueError(f"plan_terms: {key!r} is in the terminal term twice: read it with sdc_get_plan_terms")
            terminal[key] = s.terminal_weight[j]
        return {k: tuple(v) for k, v in limits.items()}, terminal

    # ------------------------------------------------------------------ plan forecast
    def set_plan_forecast(self, workload=None, carbon=None, temperature=None, wet_bulb=None, values=None):
        """What the rollouts of every later `plan`, `plan_cem` and `plan_cem_groups` believe the traces of the steps ahead are, kept on
        the engine (sdc_set_plan_forecast) until it is cleared.  Without one the planners have perfect foresight: their rollouts read
        the real workload, carbon intensity, dry bulb (with the weather noise the episode drew) and wet bulb of the next K steps --
        an oracle bound, not a controller.  Per channel a mode, by name or code (dc_rl_amd._lib.FORECAST_MODES):
          "perfect" (or None)  the truth, the channel is left alone;
          "persistence"        the value at the current step, for the whole horizon;
          "daily"              the value 96 steps (a day) earlier; the current value now -- and, for temperature / wet_bulb, wherever
                               a day earlier lies before the episode's start;
          "values"             `values`: a float64 device tensor [J, n_envs, 4], J >= K + 2, columns (workload, carbon, temperature,
                               wet_bulb), entry j what the trace is believed to be j steps ahead (j = 0: now).  The engine keeps the
                               tensor and reads it at every plan call: refresh its contents in place between decisions
                               (`future_traces(J)` gives the truth to put an error model on).  Not clipped: a workload outside
                               [0, 1] raises the workload fault in the rollouts, as a step does.
        `set_plan_forecast(None)` / no arguments / every channel "perfect": cleared, the plan calls launch what they launch without.
        A plan call overlays the step inputs in the envs' feature rows of the next K steps behind its mark and puts the saved bits
        back before it returns (three more launches per call); the rows' observation entries stay the truth, so a slot on a built-in
        rule-based policy keeps reading the true observation features.  Replicas of a group (`plan_cem_groups`) must be given
        identical `values`.  Host state: nothing is enqueued.  While a forecast is set the plan calls also refuse (ValueError) envs
        whose feature rows are stale (a set_state since their reset) and `values` with fewer than K + 2 entries.  ValueError, with the
        forecast set before still in force, for an unknown mode, and "values" without a fitting tensor."""
        modes = A.forecast_modes("set_plan_forecast", workload=workload, carbon=carbon, temperature=temperature, wet_bulb=wet_bulb)
        if values is not None:
            A.device_tensor(values, "set_plan_forecast", "values", self.torch.float64, (A.SOME, self.n_envs, 4), "(J, n_envs, 4)", self.device)
        self._set_plan_forecast_state(modes, values)

    def _set_plan_forecast_state(self, modes, values):
        """(the four codes, the values tensor or None) -> the library; the tensor is kept alive for as long as it is set"""
        s = L.SdcPlanForecast()
        s.mode[:] = modes
        if values is not None:
            s.values_entries, s.values = int(values.shape[0]), values.data_ptr()
        clear = values is None and not any(modes)
        self._call(self.lib.sdc_set_plan_forecast, None if clear else C.byref(s), refuses=True)
        self._forecast_values = values

    def _plan_forecast_state(self):
        """(codes, values) as the library holds them (what a copy of this engine is given, with `values` cloned)"""
        s = L.SdcPlanForecast()
        self._call(self.lib.sdc_get_plan_forecast, C.byref(s), refuses=True)
        kept = self._forecast_values
        if (s.values or 0) != (0 if kept is None else kept.data_ptr()):
            raise ValueError("plan_forecast: the values array was set through the C ABI: read it with sdc_get_plan_forecast")
        return list(s.mode), kept

    @property
    def plan_forecast(self):
        """The forecast in force, read back from the library (sdc_get_plan_forecast) -> the dict of `set_plan_forecast`'s arguments
        (mode names; `values` the tensor the engine keeps, or None), so that `set_plan_forecast(**e.plan_forecast)` sets the same."""
        modes, values = self._plan_forecast_state()
        return dict(A.forecast_mode_names(modes), values=values)

    def _traces(self, who, n, truth):
        n = int(n)
        A.forecast_entries(who, n, self.steps_to_episode_end())
        out = self.torch.empty((n, self.n_envs, 4), dtype=self.torch.float64, device=self.device)
        self._behind_torch_stream()      # (a "values" tensor the caller has just refreshed with torch ops)
        self._call(self.lib.sdc_forecast_traces, n, 1 if truth else 0, _p(out), self._stream(), refuses=True,
                   wrote=(out, self._forecast_values))
        return out

    def future_traces(self, n: int):
        """The true traces of the next steps -> float64 device tensor [n, n_envs, 4], columns (workload, carbon, temperature, wet_bulb),
        entry j the value j steps ahead (j = 0: what the next step reads): what a perfect forecast is, and what a caller's own error
        model for `set_plan_forecast(values=)` starts from.  n <= steps_to_episode_end() + 2 and MARK_MAX_STEPS + 2 (ValueError)."""
        return self._traces("future_traces", n, True)

    def forecast_traces(self, n: int):
        """What the forecast in force (`set_plan_forecast`) gives from the current state: `future_traces`' layout; the same tensor
        where every channel is "perfect".  A plan call of K steps plans against forecast_traces(K + 2)."""
        return self._traces("forecast_traces", n, False)

    @staticmethod
    def _three(who, name, values):
        """`values` as three ints (ls, dc, bat)"""
        three = [int(x) for x in values]
        if len(three) != 3:
            raise ValueError(f"{who}: {name} must be three integers (ls, dc, bat), got {len(three)}")
        return three

    def _cem_fixed(self, who, fixed_action, seed, draw):
        """fixed_action as three ints; the ValueErrors every CEM call raises first"""
        fixed = self._three(who, "fixed_action", fixed_action)
        if not 0 <= int(seed) < 1 << 64 or not 0 <= int(draw) < 1 << 32:
            raise ValueError(f"{who}: seed must fit 64 bits and draw 32, both unsigned")
        return fixed

    @staticmethod
    def _cem_shared(cem, n_iters, iter0, n_elite, fixed, seed, draw, alpha, p_min):
        """the fields sdc_cem_params and sdc_cem_group_params share"""
        cem.n_iters, cem.iter0, cem.n_elite = int(n_iters), int(iter0), int(n_elite)
        cem.fixed_action[:] = fixed
        cem.draw, cem.seed, cem.alpha, cem.p_min = int(draw), int(seed), float(alpha), float(p_min)

    def _group_base(self, who, R, grouped, group_base):
        """a groups call's `group_base` (None: env_index_base // R, refused where R does not divide it) as an int that fits 32 bits"""
        if group_base is None:
            base = int(self.config["env_index_base"])
            if grouped and base % R:
                raise ValueError(f"{who}: group_size = {R} does not divide env_index_base = {base} (pass group_base)")
            group_base = base // R if grouped else 0
        if not -(1 << 31) <= int(group_base) < 1 << 31:
            raise ValueError(f"{who}: group_base must fit 32 bits")
        return int(group_base)

    def _cem(self, who, fn, cem, fixed, K, lead, outputs, result, sized, check, sizes, n_iters, n_elite, probs, best_seq, seed, draw, iter0,
             alpha, p_min, reward_weights, gamma, info_weights):
        """The CEM call of plan_cem and plan_cem_groups: library function `fn` with `cem`, its params struct with the caller's own
        fields set (the shared ones are filled here), probs [K, lead, 3, 3] / best_seq [K, lead, 3] -- a caller's are validated if
        `check` -- and, behind them, new tensors of `outputs`' (shape, dtype); -> result(*the arrays in the library's order).  Not
        `sized` (sizes no array can be given): the library is called with null arrays and words the refusal; it looks at the sizes
        before the arrays."""
        t = self.torch
        if check and probs is not None:
            A.device_tensor(probs, who, "probs", t.float64, (K, lead, 3, 3), device=self.device)
        if check and best_seq is not None:
            A.device_tensor(best_seq, who, "best_seq", t.int32, (K, lead, 3), device=self.device)
        obj = plan_objective(reward_weights, gamma, info_weights)
        self._cem_shared(cem, n_iters, iter0, n_elite, fixed, seed, draw, alpha, p_min)
        arrays = []
        if sized:
            # (probs and best_seq -- the defaults below, a caller's, CEMMPCAgent's shifted ones -- are read by the sample kernel)
            self._behind_torch_stream()
            if probs is None:
                probs = t.full((K, lead, 3, 3), 1.0 / 3.0, dtype=t.float64, device=self.device)
            if best_seq is None:
                best_seq = t.tensor([1, 1, 2], dtype=t.int32, device=self.device).expand(K, lead, 3).contiguous()
            arrays = [probs, best_seq] + [t.empty(shape, dtype=dtype, device=self.device) for shape, dtype in outputs]
        ptrs = [_p(x) for x in arrays] or [None] * (2 + len(outputs))
        self._call(fn, K, C.byref(cem), C.byref(obj), *ptrs, *self._obs_ptrs, self._stream(), refuses=True, wrote=arrays)
        if not sized:
            raise L.SdcError(f"{who}: {fn.__name__} accepted {sizes} and no arrays")
        return result(*arrays)

    def plan_cem(self, horizon: int, n_iters: int, n_candidates: int, n_elite: int, *, probs=None, best_seq=None, seed: int = 0,
                 draw: int = 0, iter0: int = 0, alpha: float = 0.0, p_min: float = 0.0, fixed_action=(-1, -1, -1),
                 reward_weights=(1.0, 1.0, 1.0), gamma: float = 1.0, info_weights=None) -> CEMResult:
        """Plan `horizon` = K steps ahead with the cross-entropy method and come back (sdc_plan_cem): one library call -- one mark, then
        per iteration: sample M = n_candidates sequences on the device from every env's per-step, per-agent categorical distribution,
        score them as `plan` does (the same objective arguments), refit the distribution to the E = n_elite best, keep the best
        sequence found so far -- with no Python between the launches.  `probs` float64 device tensor [K, N, 3 agents, 3 actions]
        (None: uniform) and `best_seq` int32 [K, N, 3], the incumbent (None: do nothing -- 1, 1, 2); tensors passed in are updated in
        place and returned, and their entries are not checked (they live on the device).  Candidate 0 of every iteration is the
        incumbent, so its score never falls and it wins ties.  The draws are the project's counter-based generator keyed on (seed, draw,
        iteration index iter0 + i, candidate, step, the env's GLOBAL index): the same arguments give the same candidates, whatever the
        batch is split into; a caller numbers its decisions with `draw`, and a call of I iterations equals I calls of one with iter0 =
        0 .. I-1 that carry probs and best_seq.  Refit: p = normalise(max(alpha * p + (1 - alpha) * elite frequency, p_min)) (the
        exact operations: include/sustaindc_hip.h).  fixed_action: per agent -1, or the value 0..2 every sampled candidate carries
        for it (its probs stay as they are).  -> CEMResult(action [N, 3] = best_seq[0], best_seq, best_score [I, N], probs, cand
        [M, K, N, 3], cand_score [M, N]).  The engine afterwards, and the price (the envs' one live mark), are `plan`'s.  ValueError,
        with the engine untouched, for malformed tensors or objective and what the library refuses: plan's horizon, auto-reset and
        verify-mode rules; n_iters < 1, iter0 < 0, iter0 + n_iters > 65536; M outside [2, CEM_MAX_CAND]; E outside [1, M]; a
        fixed_action outside [-1, 2]; alpha outside [0, 1); p_min outside [0, 1/3]."""
        t = self.torch
        K, N, M, n_it = int(horizon), self.n_envs, int(n_candidates), int(n_iters)
        fixed = self._cem_fixed("plan_cem", fixed_action, seed, draw)
        cem = L.SdcCemParams()
        cem.n_cand = M
        sized = 1 <= K <= L.MARK_MAX_STEPS and 2 <= M <= L.CEM_MAX_CAND and n_it >= 1 and 0 <= int(iter0) <= L.CEM_MAX_ITERS - n_it
        outputs = [((n_it, N), t.float64), ((N, 3), t.int32), ((M, K, N, 3), t.int32), ((M, N), t.float64)]
        return self._cem("plan_cem", self.lib.sdc_plan_cem, cem, fixed, K, N, outputs,
                         lambda probs, best_seq, best_score, action, cand, cand_score:
                         CEMResult(action, best_seq, best_score, probs, cand, cand_score),
                         sized, True, f"K = {K}, M = {M}, I = {n_it}, iter0 = {int(iter0)}", n_it, n_elite, probs, best_seq, seed, draw,
                         iter0, alpha, p_min, reward_weights, gamma, info_weights)

    def sync_groups(self, group_size: int):
        """Every group of `group_size` consecutive envs becomes a copy of its first env: one clone_envs call with the leaders as sources
        (the replicas finish the leader's episode exactly; their own resets stay keyed on their own global indices, so call this again
        after a reset or auto-reset).  What plan_cem_groups asks of the batch.  ValueError for a group_size that is not in [2, n_envs]
        or does not divide n_envs, and what clone_envs refuses.  -> (obs, share_obs) views."""
        return self.clone_envs(*group_sync_pairs(group_size, self.n_envs, "n_envs"))

    def plan_cem_groups(self, group_size: int, horizon: int, n_iters: int, n_elite: int, *, probs=None, best_seq=None, seed: int = 0,
                        draw: int = 0, iter0: int = 0, alpha: float = 0.0, p_min: float = 0.0, fixed_action=(-1, -1, -1),
                        group_base: Optional[int] = None, reward_weights=(1.0, 1.0, 1.0), gamma: float = 1.0,
                        info_weights=None) -> GroupCEMResult:
        """`plan_cem` with the candidates in env slots (sdc_plan_cem_groups): the batch is G = N / R groups of R = group_size
        consecutive envs that hold ONE state (`sync_groups` makes them so; stepping with the result's `step_actions` keeps them so),
        and in every iteration each replica plays its own sampled sequence in a single K = horizon step rollout of the whole batch --
        one sample launch, one rollout, one score, one rewind and one refit per iteration whatever R is, up to CEM_MAX_GROUP = 1024
        samples per group.  The arithmetic is plan_cem's with "candidate m of env n" read as "replica r of group g": for R <= 64 the
        results equal, bit for bit, plan_cem(n_candidates=R) on an engine of G envs whose env g is group g's state and whose
        env_index_base is `group_base`.  `probs` float64 device tensor [K, G, 3, 3] (None: uniform) and `best_seq` int32 [K, G, 3]
        (None: do nothing -- 1, 1, 2) are updated in place and returned; replica 0 of a group carries the incumbent.  `group_base`:
        the global index of this engine's group 0 in the generator's counter (None: env_index_base // R, refused where R does not
        divide env_index_base).  The other arguments, the engine afterwards and the price (the envs' one live mark) are plan_cem's.
        What the host knows of a group's replicas (episode step, config, location, feature-row flag) is checked; bit equality of their
        states beyond that is the caller's contract.  -> GroupCEMResult(action [G, 3], step_actions [N, 3], best_seq, best_score
        [I, G], probs, cand [K, N, 3], cand_score [N]).  ValueError, with the engine untouched, for malformed tensors or objective and
        what the library refuses: plan_cem's rules with n_candidates read as group_size; R outside [2, CEM_MAX_GROUP] or not dividing
        N; E outside [1, R]; a negative group_base; a group out of step."""
        t = self.torch
        K, N, R, n_it = int(horizon), self.n_envs, int(group_size), int(n_iters)
        fixed = self._cem_fixed("plan_cem_groups", fixed_action, seed, draw)
        grouped = 2 <= R <= L.CEM_MAX_GROUP and N % R == 0
        G = N // R if grouped else 0
        cem = L.SdcCemGroupParams()
        cem.group_size, cem.group_base = R, self._group_base("plan_cem_groups", R, grouped, group_base)
        sized = grouped and 1 <= K <= L.MARK_MAX_STEPS and n_it >= 1 and 0 <= int(iter0) <= L.CEM_MAX_ITERS - n_it
        outputs = [((n_it, G), t.float64), ((G, 3), t.int32), ((N, 3), t.int32), ((K, N, 3), t.int32), ((N,), t.float64)]
        return self._cem("plan_cem_groups", self.lib.sdc_plan_cem_groups, cem, fixed, K, G, outputs,
                         lambda probs, best_seq, best_score, action, step_actions, cand, cand_score:
                         GroupCEMResult(action, step_actions, best_seq, best_score, probs, cand, cand_score),
                         sized, sized, f"R = {R}, K = {K}, I = {n_it}, iter0 = {int(iter0)}", n_it, n_elite, probs, best_seq, seed, draw,
                         iter0, alpha, p_min, reward_weights, gamma, info_weights)

    def _stats_into(self, who, into, policy_stats=None, plan_stats=None, groups=None):
        """the EpisodeStats a statistics call fills: a new one, or the caller's `into` checked (ValueError in `who`'s name) -- tensors of
        this engine's shapes on its device, a PolicyStats exactly when `policy_stats` (None: the call has none) and a PlanStats exactly
        when `plan_stats` (the same); `groups` = G: the PlanStats is per group and carries `diverged`"""
        t, N = self.torch, self.n_envs
        want = ((t.float64, (L.STATS_FIELDS, N, L.INFO_DIM)), (t.float64, (N, L.N_AGENTS)), (t.int32, (N, 2)))     # stats, returns, counts
        pwant = ((t.int32, (N, L.N_AGENTS, L.POLICY_COUNTS)), (t.float64, (N, L.N_AGENTS, L.POLICY_SUMS)))        # counts, sums
        mwant = ((t.int32, (N, L.N_AGENTS, L.POLICY_COUNTS)), (t.float64, (N, L.PLAN_SUMS)))                      # the plan's counts, sums
        if groups is not None:                                                                                    # ... per group, and diverged
            mwant = ((t.int32, (groups, L.N_AGENTS, L.POLICY_COUNTS)), (t.float64, (groups, L.PLAN_SUMS)), (t.int32, (groups,)))
        new = lambda shapes: [t.empty(sh, dtype=d, device=self.device) for d, sh in shapes]
        if into is None:
            return EpisodeStats(*new(want), PolicyStats(*new(pwant)) if policy_stats else None,
                                plan=PlanStats(*new(mwant)) if plan_stats else None)
        fits = lambda xs, shapes: all(A.is_tensor(x, d, sh, self.device, cuda=False) for x, (d, sh) in zip(xs, shapes))
        if not (isinstance(into, EpisodeStats) and fits((into.stats, into.returns, into.counts), want)):
            raise ValueError(f"{who}: into must be an EpisodeStats of this engine (contiguous tensors on {self.device}: stats "
                             f"float64 {want[0][1]}, returns float64 {want[1][1]}, counts int32 {want[2][1]})")
        if policy_stats is not None:
            pol = into.policy
            if policy_stats != (pol is not None):
                raise ValueError(f"{who}: into must carry a PolicyStats exactly when policy_stats is set (policy_stats = "
                                 f"{bool(policy_stats)}, into.policy is {'given' if pol is not None else 'None'})")
            if pol is not None and not (isinstance(pol, PolicyStats) and fits((pol.counts, pol.sums), pwant)):
                raise ValueError(f"{who}: into.policy must be a PolicyStats of this engine (contiguous tensors on {self.device}: counts "
                                 f"int32 {pwant[0][1]}, sums float64 {pwant[1][1]})")
        if plan_stats is not None:
            pl = into.plan
            if plan_stats != (pl is not None):
                raise ValueError(f"{who}: into must carry a PlanStats exactly when plan_stats is set (plan_stats = "
                                 f"{bool(plan_stats)}, into.plan is {'given' if pl is not None else 'None'})")
            if pl is not None and not (isinstance(pl, PlanStats) and fits((pl.counts, pl.sums, pl.diverged), mwant)):
                raise ValueError(f"{who}: into.plan must be a PlanStats of this engine (contiguous tensors on {self.device}: counts "
                                 f"int32 {mwant[0][1]}, sums float64 {mwant[1][1]}" +
                                 (f", diverged int32 {mwant[2][1]})" if groups is not None else ")"))
        self._behind_torch_stream()      # (its tensors may have been touched on torch's current stream)
        return into

    def rollout_stats(self, actions=None, n_steps: int = None, into: Optional[EpisodeStats] = None) -> EpisodeStats:
        """K env-steps as `rollout` takes them, reduced on the device to per-env statistics (sdc_rollout_stats): the steps' outputs go
        into a block the engine's library owns, in chunks, and one small kernel per chunk folds them into an EpisodeStats -- sum, min,
        max and count of positive values of all 44 info columns, the three agents' returns, the step count, the OR of the fault bits --
        so an episode of a large batch never materialises its 617 B per env-step.  fp64, in step order (the exact operations:
        include/sustaindc_hip.h).  actions: int32 device tensor [K, N, 3], or None with n_steps when every slot has a built-in
        policy; K may reach the episode's end (steps_to_episode_end()), where the auto-reset happens as in `rollout`.  `into`: an
        EpisodeStats of this engine to continue (its tensors are updated in place and it is returned); calls split anywhere give the
        bits of one call.  The engine moves; its single-step views (obs, share_obs, rew, done, info, final_obs) follow the last step,
        as after `rollout`.  ValueError, with the engine untouched, for malformed arguments and what the library refuses: K < 1,
        K > steps_to_episode_end(), no reset() yet, verify mode (debug_flags DEBUG_VERIFY)."""
        K = self._sequence_steps("rollout_stats", actions, n_steps, self.device)
        res = self._stats_into("rollout_stats", into)
        self._call(self.lib.sdc_rollout_stats, K, _p(actions), 0 if into is None else 1, _p(res.stats), _p(res.returns), _p(res.counts),
                   *self._obs_ptrs, _p(self.rew), _p(self.done), _p(self.info), _p(self.final_obs), self._stream(),
                   refuses=True, wrote=(res.stats, res.returns, res.counts, actions))
        return res

    def rollout_actor_stats(self, n_steps: int, sample: bool = False, into: Optional[EpisodeStats] = None,
                            policy_stats: bool = True) -> EpisodeStats:
        """K env-steps as `rollout_actor` takes them -- the three actors (set_actor) choosing every action inside the kernel --, reduced
        on the device (sdc_rollout_actor_stats): `rollout_stats`' EpisodeStats of the environment's outputs and, in its `policy`, a
        PolicyStats of what the actors did -- per env and agent how often each action was played, how often it changed from one step to
        the next, the summed log-probability of the actions played and the summed entropy of the distributions (fp64, in step order; the
        exact operations: include/sustaindc_hip.h) -- so an evaluation of a trained policy never materialises its 617 + 48 B per
        env-step.  sample=False: the distributions' mode, True: a draw (the same draws as `rollout_actor`, however the steps are split
        into calls).  `policy_stats=False` leaves the PolicyStats out (`policy` is None; the logits are not written).  `into`: an
        EpisodeStats of this engine to continue, carrying a PolicyStats exactly when `policy_stats` is set; calls split anywhere give the
        bits of one call.  The engine moves; its single-step views follow the last step.  ValueError, with the engine untouched, for
        malformed arguments and what the library refuses: what `rollout_stats` refuses, an actor not set, actors of different
        activations, actors set after the last reset / step, a batch `rollout_actor` does not serve."""
        pol = bool(policy_stats)
        res = self._stats_into("rollout_actor_stats", into, pol)
        pc, ps = (res.policy.counts, res.policy.sums) if pol else (None, None)
        self._call(self.lib.sdc_rollout_actor_stats, int(n_steps), 1 if sample else 0, 0 if into is None else 1, _p(res.stats),
                   _p(res.returns), _p(res.counts), _p(pc), _p(ps), *self._obs_ptrs, _p(self.rew), _p(self.done), _p(self.info),
                   _p(self.final_obs), self._stream(), refuses=True, wrote=(res.stats, res.returns, res.counts, pc, ps))
        return res

    def _mpc_stats(self, who, fn, mpc, own, sized, sizes, grouped, n_steps, H, lead, outputs, left, n_iters, n_elite, probs, best_seq,
                   resume_steps, warm_start, seed, draw, alpha, p_min, fixed_action, idle_action, reward_weights, gamma, info_weights, into,
                   plan_stats):
        """The closed-loop call of rollout_cem_stats and rollout_cem_groups_stats: library function `fn` with `mpc`, its params struct --
        the loop's fields and the shared ones of its `cem` are filled here, the caller's own by own(), which raises the caller's own
        ValueErrors at their place among the others --, probs [H, lead, 3, 3] / best_seq [H, lead, 3] (a caller's are validated, None:
        new ones) and, behind them, new tensors of `outputs`' (shape, dtype), best_score and best_action first; `grouped`: the PlanStats
        is per group with `diverged`, and the third output is step_actions.  left() behind the call: the steps the episode had left at
        the first decision.  -> the EpisodeStats with its `mpc`.  Not `sized`: as in _cem."""
        t = self.torch
        fixed = self._cem_fixed(who, fixed_action, seed, draw)
        idle = self._three(who, "idle_action", idle_action)
        k_res = int(resume_steps)
        if k_res < 0 or (k_res > 0 and (probs is None or best_seq is None)):
            raise ValueError(f"{who}: resume_steps = {k_res} must not be negative, and resuming needs probs and best_seq")
        own()
        obj = plan_objective(reward_weights, gamma, info_weights)
        if sized and probs is not None:
            A.device_tensor(probs, who, "probs", t.float64, (H, lead, 3, 3), device=self.device)
        if sized and best_seq is not None:
            A.device_tensor(best_seq, who, "best_seq", t.int32, (H, lead, 3), device=self.device)
        pl = bool(plan_stats)
        res = self._stats_into(who, into, None, pl, lead if grouped and sized else None)
        mpc.horizon, mpc.warm_start, mpc.resume, mpc.resume_steps = H, 1 if warm_start else 0, 1 if k_res > 0 else 0, k_res
        mpc.idle_action[:] = idle
        self._cem_shared(mpc.cem, n_iters, 0, n_elite, fixed, seed, draw, alpha, p_min)
        arrays = [None] * (2 + len(outputs))
        if sized:
            self._behind_torch_stream()      # (a caller's probs / best_seq may have been filled by torch ops)
            new = lambda shape, dtype: t.empty(shape, dtype=dtype, device=self.device)
            arrays = [new((H, lead, 3, 3), t.float64) if probs is None else probs, new((H, lead, 3), t.int32) if best_seq is None else best_seq]
            arrays += [new(shape, dtype) for shape, dtype in outputs]
        n_plan = 3 if grouped else 2
        plan_arrays = [res.plan.counts, res.plan.sums, res.plan.diverged][:n_plan] if pl else [None] * n_plan
        self._call(fn, int(n_steps), C.byref(mpc), C.byref(obj), 0 if into is None else 1, _p(res.stats), _p(res.returns), _p(res.counts),
                   *[_p(x) for x in plan_arrays + arrays], *self._obs_ptrs, _p(self.rew), _p(self.done), _p(self.info), _p(self.final_obs),
                   self._stream(), refuses=True, wrote=[res.stats, res.returns, res.counts] + plan_arrays + arrays)
        if not sized:
            raise L.SdcError(f"{who}: {fn.__name__} accepted {sizes} and no arrays")
        plan = mpc_schedule(left(), int(n_steps), H, self.config["auto_reset"], bool(warm_start), k_res)
        res.mpc = MPCCarry(arrays[0], arrays[1], plan[-1][0], sum(1 for d in plan if d[1]), arrays[3], arrays[2],
                           arrays[4] if grouped else None)
        return res

    def rollout_cem_stats(self, n_steps: int, horizon: int, n_iters: int, n_candidates: int, n_elite: int, *, probs=None, best_seq=None,
                          resume_steps: int = 0, warm_start: bool = True, seed: int = 0, draw: int = 0, alpha: float = 0.0,
                          p_min: float = 0.0, fixed_action=(-1, -1, -1), idle_action=(1, 1, 2), reward_weights=(1.0, 1.0, 1.0),
                          gamma: float = 1.0, info_weights=None, into: Optional[EpisodeStats] = None,
                          plan_stats: bool = True) -> EpisodeStats:
        """n_steps env-steps under receding-horizon control with the cross-entropy method, reduced on the device
        (sdc_rollout_cem_stats): before every step the library plans as `plan_cem(K, n_iters, n_candidates, n_elite, ...)` does -- K =
        `horizon` cut to what the episode has left, as CEMMPCAgent cuts it --, plays the best sequence's first action, and folds the
        step into `rollout_stats`' EpisodeStats; one library call with no Python between the decisions.  What CEMMPCAgent does in a
        loop of act() and step(), bit for bit: the decision schedule (planned or idle, fresh or warm-started from the last result moved
        up by a step, draw + j for the j-th planned decision) is written out in include/sustaindc_hip.h.  The result's `plan` is a
        PlanStats -- per env and agent the actions played, per env the predicted score, its gain over the iterations and the number of
        planned / idle decisions (`plan_stats=False`: None) --, its `mpc` an MPCCarry.  `probs` float64 [horizon, N, 3, 3] and
        `best_seq` int32 [horizon, N, 3]: the planner's arrays (None: new ones); with `resume_steps` = k > 0 they hold an earlier
        decision's unshifted result of k steps (an earlier call's `mpc`), and the first planned decision continues from it.
        `idle_action`: what an idle decision plays and a fresh incumbent holds.  seed, alpha, p_min, fixed_action and the objective:
        `plan_cem`'s; plan terms and a plan forecast set on the engine apply to every decision.  `into`: an EpisodeStats of this
        engine to continue, carrying a PlanStats exactly when `plan_stats` is set.  The engine moves; its single-step views follow the
        last step; the envs' live mark is used up.  n_steps may reach the episode's end, where the auto-reset happens.  ValueError,
        with the engine untouched, for malformed arguments and what the library refuses: what `rollout_stats` and `plan_cem` refuse
        (the latter's horizon rules replaced by the schedule), horizon outside [1, MARK_MAX_STEPS], resume_steps outside [0, horizon]
        or without the arrays, an idle_action outside 0..2."""
        t = self.torch
        H, N, M, n_it = int(horizon), self.n_envs, int(n_candidates), int(n_iters)
        mpc = L.SdcMpcParams()

        def own():
            mpc.cem.n_cand = M

        sized = 1 <= H <= L.MARK_MAX_STEPS and 2 <= M <= L.CEM_MAX_CAND and 1 <= n_it <= L.CEM_MAX_ITERS
        outputs = [((n_it, N), t.float64), ((N, 3), t.int32), ((M, H, N, 3), t.int32), ((M, N), t.float64)]
        left = self.steps_to_episode_end()
        return self._mpc_stats("rollout_cem_stats", self.lib.sdc_rollout_cem_stats, mpc, own, sized, f"H = {H}, M = {M}, I = {n_it}", False,
                               n_steps, H, N, outputs, lambda: left, n_it, n_elite, probs, best_seq, resume_steps, warm_start, seed, draw,
                               alpha, p_min, fixed_action, idle_action, reward_weights, gamma, info_weights, into, plan_stats)

    def rollout_cem_groups_stats(self, n_steps: int, group_size: int, horizon: int, n_iters: int, n_elite: int, *, sync: bool = False,
                                 probs=None, best_seq=None, resume_steps: int = 0, warm_start: bool = True, seed: int = 0, draw: int = 0,
                                 alpha: float = 0.0, p_min: float = 0.0, fixed_action=(-1, -1, -1), idle_action=(1, 1, 2),
                                 group_base: Optional[int] = None, reward_weights=(1.0, 1.0, 1.0), gamma: float = 1.0, info_weights=None,
                                 into: Optional[EpisodeStats] = None, plan_stats: bool = True) -> EpisodeStats:
        """`rollout_cem_stats` over replica groups (sdc_rollout_cem_groups_stats): before every step the library plans as
        `plan_cem_groups(group_size, K, n_iters, n_elite, ...)` does -- G = N / R groups of R = group_size consecutive envs that hold
        one state, one rollout of the batch per iteration --, plays the result's `step_actions`, folds the step into the EpisodeStats
        and checks on the device that every replica's rew, done and info rows (without info[reserved]) still equal its group's first
        env's, bit for bit; one library call with no Python between the decisions.  What GroupCEMMPCAgent does in a loop of act() and
        step(), bit for bit.  `sync=True`: the call begins with `sync_groups(group_size)` inside the library, and its first planned
        decision starts fresh (ValueError together with `resume_steps`); without it the groups must be in step, as for
        `plan_cem_groups`.  n_steps <= steps_to_episode_end() puts an auto-reset at the call's last step at most -- the replicas
        draw resets of their own there --, so a call per episode with `sync=True` is all an evaluation needs.  The statistics stay per
        env [N] (a group's replicas carry equal rows: read every R-th); the result's `plan` is a PlanStats PER GROUP -- counts
        [G, 3, 5], sums [G, 4] and `diverged` int32 [G], the (step, replica) pairs that differed from their group's first env
        (`plan_stats=False`: None, and nothing is checked) --, its `mpc` an MPCCarry per group with `step_actions` [N, 3].  `probs`
        float64 [horizon, G, 3, 3], `best_seq` int32 [horizon, G, 3], `resume_steps`, `idle_action`, `into` and the other arguments:
        `rollout_cem_stats`' and `plan_cem_groups`'.  ValueError, with the engine untouched, for malformed arguments and what the
        library refuses: what `rollout_cem_stats` refuses, what `plan_cem_groups` refuses about the groups."""
        t = self.torch
        who = "rollout_cem_groups_stats"
        H, N, R, n_it = int(horizon), self.n_envs, int(group_size), int(n_iters)
        grouped = 2 <= R <= L.CEM_MAX_GROUP and N % R == 0
        G = N // R if grouped else 0
        mpc = L.SdcMpcGroupParams()

        def own():
            mpc.sync_first = 1 if sync else 0
            mpc.cem.group_size, mpc.cem.group_base = R, self._group_base(who, R, grouped, group_base)

        def left():
            # behind the sync, from where the call has left the batch (no env finished: it moved n_steps)
            return int(n_steps) if self.last_done() is not None else self.steps_to_episode_end() + int(n_steps)

        sized = grouped and 1 <= H <= L.MARK_MAX_STEPS and 1 <= n_it <= L.CEM_MAX_ITERS
        outputs = [((n_it, G), t.float64), ((G, 3), t.int32), ((N, 3), t.int32), ((H, N, 3), t.int32), ((N,), t.float64)]
        return self._mpc_stats(who, self.lib.sdc_rollout_cem_groups_stats, mpc, own, sized, f"R = {R}, H = {H}, I = {n_it}", True, n_steps, H,
                               G, outputs, left, n_it, n_elite, probs, best_seq, resume_steps, warm_start, seed, draw, alpha, p_min,
                               fixed_action, idle_action, reward_weights, gamma, info_weights, into, plan_stats)

    def evaluate(self, n_episodes: int, actions=None, *, actors: bool = False, sample: bool = False, mpc=None) -> EpisodeStats:
        """`n_episodes` whole episodes of the batch, one `rollout_stats` of episode_steps steps each -> an EpisodeStats whose tensors
        carry a leading [E] dimension (stats [E, 4, N, 44], returns [E, N, 3], counts [E, N, 2]).  The batch is reset first; between
        episodes the auto-reset starts the next one (auto_reset off: reset() is called).  actions: None (every slot on a built-in
        policy), an int32 device tensor [episode_steps, N, 3] replayed every episode, or a callable episode -> such a tensor.
        `actors=True`: the three actors (set_actor) play instead -- one `rollout_actor_stats` per episode, `sample` as there -- and
        the result's `policy` is a PolicyStats with the same leading dimension; ValueError together with `actions`.  `mpc=agent`: a
        CEMMPCAgent plans every step -- one `agent.rollout_stats` (`rollout_cem_stats`) per episode, the agent's draw counter running
        on from episode to episode -- and the result's `plan` is a PlanStats with the same leading dimension; ValueError together with
        `actions` or `actors`.  A GroupCEMMPCAgent plans over replica groups (`rollout_cem_groups_stats`, one call per episode, each
        with `sync=True`: the replicas drew resets of their own); the PlanStats is then per group and carries `diverged`."""
        t = self.torch
        E = int(n_episodes)
        if E < 1:
            raise ValueError(f"evaluate: n_episodes = {n_episodes} must be positive")
        if actors and actions is not None:
            raise ValueError("evaluate: actors=True plays the actors' own actions: give no actions")
        if mpc is not None and (actors or actions is not None):
            raise ValueError("evaluate: mpc= plays the planner's own actions: give neither actions nor actors")
        if mpc is not None and not callable(getattr(mpc, "rollout_stats", None)):
            raise ValueError("evaluate: mpc must be an agent with rollout_stats(env, n_steps) (dc_rl_amd.agents.CEMMPCAgent)")
        if mpc is None and not actors and actions is None and any(p == 0 for p in self.policy):
            raise ValueError("evaluate: actions=None needs a built-in policy on every agent slot")
        self.reset()
        eps = []
        for e in range(E):
            if e > 0 and not self.config["auto_reset"]:
                self.reset()
            if mpc is not None:
                eps.append(mpc.rollout_stats(self, self.episode_steps))
            elif actors:
                eps.append(self.rollout_actor_stats(self.episode_steps, sample=sample))
            else:
                a = actions(e) if callable(actions) else actions
                eps.append(self.rollout_stats(a, n_steps=self.episode_steps))
        stack = lambda get: t.stack([get(x) for x in eps])
        pol = PolicyStats(stack(lambda x: x.policy.counts), stack(lambda x: x.policy.sums)) if actors else None
        pln = None
        if mpc is not None:
            pln = PlanStats(stack(lambda x: x.plan.counts), stack(lambda x: x.plan.sums),
                            stack(lambda x: x.plan.diverged) if eps[0].plan.diverged is not None else None)
        return EpisodeStats(stack(lambda x: x.stats), stack(lambda x: x.returns), stack(lambda x: x.counts), pol, plan=pln)

    def profile(self, every: int = 1):
        """Per-kernel HIP-event timing on the launch stream (measurement only): every k-th step, 0 = off."""
        self._call(self.lib.sdc_profile_enable, int(every))

    def profile_read(self, reset: bool = True) -> dict:
        out = (C.c_double * 5)()
        self._call(self.lib.sdc_profile_read, out, 1 if reset else 0)
        return {"dynamics_ms": out[0], "reward_ms": out[1], "reset_ms": out[2], "steps": int(out[3]),
                "resets": int(out[4])}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.sdc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
