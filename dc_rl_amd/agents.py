"""Rule-based baseline agents of the reference (utils/base_agents.py, utils/rbc_agents.py) with the same class and
method names, plus batched device-side versions (`act_batch`) that produce actions for N environments from torch
tensors without leaving the GPU.

Action encodings (sustaindc_env.py, envs/*):  load shifting {0 defer, 1 do nothing, 2 process the queue};
HVAC set-point {0 down, 1 hold, 2 up};  battery {0 charge, 1 discharge, 2 idle}.
"""
from __future__ import annotations

import numpy as np


class BaseLoadShiftingAgent:
    """utils/base_agents.py:3-27 -- always 'do nothing' (1)."""

    def __init__(self, parameters=None):
        self.parameters = parameters
        self.do_nothing_action_value = 1

    def do_nothing_action(self):
        return self.do_nothing_action_value

    def act(self, *args, **kwargs):
        return self.do_nothing_action()

    def act_batch(self, n_envs, device=None):
        import torch
        return torch.full((n_envs,), self.do_nothing_action_value, dtype=torch.int32, device=device)


class BaseHVACAgent(BaseLoadShiftingAgent):
    """utils/base_agents.py:29-58 -- always 'hold the set-point' (1).  The reference class has no `act()` although
    sustaindc_env.py:640 calls it when agent_dc is not trained (AttributeError there); here `act()` returns the
    do-nothing action, which is what that call site means."""

    def __init__(self, parameters=None):
        self.parameters = parameters
        self.do_nothing_action_value = np.int64(1)


class BaseBatteryAgent(BaseLoadShiftingAgent):
    """utils/base_agents.py:60-98 -- always 'idle' (2)."""

    def __init__(self, parameters=None):
        self.parameters = parameters
        self.do_nothing_action_value = 2


class RBCBatteryAgent:
    """utils/rbc_agents.py:3-48 -- charge (0) when the smoothed carbon-intensity forecast `look_ahead` steps ahead is
    above the current value, else discharge (1)."""

    def __init__(self, look_ahead=3, smooth_window=1, max_soc=0.9, min_soc=0.2):
        self.look_ahead = look_ahead
        self.smooth_window = smooth_window
        self.max_soc = max_soc
        self.min_soc = min_soc

    def act(self, carbon_intensity_values, current_soc):
        window = self.smooth_window
        smoothed = np.convolve(carbon_intensity_values, np.ones(window), "valid") / window
        return 0 if smoothed[self.look_ahead] > carbon_intensity_values[0] else 1

    def act_batch(self, carbon_intensity_values, current_soc=None):
        """carbon_intensity_values: torch tensor [N, K] (current value first, then the forecast) -> int32 [N]."""
        import torch
        w = self.smooth_window
        x = carbon_intensity_values
        sm = x.unfold(1, w, 1).sum(-1) / w if w > 1 else x
        return torch.where(sm[:, self.look_ahead] > x[:, 0], 0, 1).to(torch.int32)


class trim_and_respond_ctrl:
    """utils/trim_and_respond.py:8-38 -- "trim and respond" supply-air reset for agent_dc: while the monitored
    temperature stays at or below the limit, hold the set-point (1) and every fifth consecutive call trim it up (2);
    above the limit respond by lowering it (0).  Same class name, constructor arguments and `action()` as the reference."""

    def __init__(self, TandR_monitor_idx=6, TandR_monitor: str = "avg_room_temp", TandR_monitor_limit: float = 27):
        assert (TandR_monitor == "avg_room_temp") | (TandR_monitor == "crac_return_temp"), \
            f"invalid TandR_monitor monitor string : {TandR_monitor}"
        self.TandR_monitor = TandR_monitor
        self.TandR_monitor_limit = TandR_monitor_limit
        self.TandR_monitor_idx = TandR_monitor_idx
        self.response_duration_counter = 0
        self.response_duration_limit = 4  # 1 hour at a 15-minute sampling interval

    def set_limit(self, x):
        self.TandR_monitor_limit = x

    def action(self, obs):
        curr_val = obs
        if self.TandR_monitor_limit >= curr_val:
            if self.response_duration_counter > self.response_duration_limit:
                self.response_duration_counter = 0
                return 2
            self.response_duration_counter += 1
            return 1
        return 0


# Device-side counterparts: `SdcEngine(policy=(ls, dc, bat))` / sdc_config.policy run these inside the step kernel
# (include/sustaindc_hip.h enum sdc_policy), so `SdcEngine.rollout_policy` plays whole episodes closed-loop without an
# action array:
#   BaseLoadShiftingAgent / BaseHVACAgent / BaseBatteryAgent -> POLICY_DO_NOTHING on that slot
#   RBCBatteryAgent(look_ahead=3, smooth_window=1)           -> POLICY_RBC on the battery slot: fed [ci, ci_future...] of the
#                                                               env's `infos["__common__"]` (sustaindc_env.py:601-603)
#   trim_and_respond_ctrl(limit)                              -> POLICY_TRIM_AND_RESPOND on the dc slot: fed the
#                                                               dc_int_temperature the previous step reported
POLICY_EXTERNAL, POLICY_DO_NOTHING, POLICY_RBC, POLICY_TRIM_AND_RESPOND = 0, 1, 2, 3


def _mpc_horizon(env, horizon):
    """What every MPC agent's decision starts from: env an SdcEngine or a SustainDCVecEnv -> (the horizon cut to what the episode has
    left -- the planner does not look across an episode's end; 0: fewer than two steps left, do nothing --, the episode step)"""
    eng = getattr(env, "engine", env)
    left = eng.steps_to_episode_end()
    K = min(horizon, left - 1 if eng.config["auto_reset"] else left)
    return (K if left >= 2 and K >= 1 else 0), eng.config["episode_steps"] - left


def _set_forecast(env, forecast):
    """an MPC agent's `forecast` onto the env's engine: a mode's name for all four channels, or the dict of set_plan_forecast's arguments"""
    if isinstance(forecast, str):
        forecast = dict(workload=forecast, carbon=forecast, temperature=forecast, wet_bulb=forecast)
    env.set_plan_forecast(**forecast)


def _do_nothing(env, values):
    """the do-nothing actions `values` (ls, dc, bat) for every env: int32 [N, the env's agent columns] on the env's device"""
    import torch
    eng = getattr(env, "engine", env)
    idx = list(getattr(env, "_agent_idx", (0, 1, 2)))
    return torch.tensor([values[i] for i in idx], dtype=torch.int32, device=eng.device).expand(eng.n_envs, len(idx)).contiguous()


class ShootingMPCAgent:
    """Random-shooting model-predictive control with the simulator as its own model: at every decision draw `n_candidates` action
    sequences of `horizon` steps per env, score them on the device from the env's current state (SdcEngine.plan / SustainDCVecEnv.plan
    over sdc_plan: mark, roll out, score, rewind) and play the first action of the best.  Candidate 0 is always the do-nothing sequence
    (ls 1, dc 1, bat 2), so on the model the chosen sequence never scores below doing nothing.  The candidates come from a torch.Generator on
    the env's device seeded with `seed`: two agents with one seed on twin envs choose the same actions.  reward_weights, gamma,
    info_weights: the objective, as `plan` takes it.  The horizon is shortened to what the episode has left (the planner does not look
    across an episode's end); with fewer than two steps left the agent does nothing.  `last`: the latest PlanResult (None after a
    do-nothing fallback), `last_horizon` the horizon it used.  The agent plans through the env, so limits and a terminal term:
    `env.set_plan_terms`, and a learned value at the horizon's end: `env.set_critic` + `env.set_plan_critic` (no argument here: the term
    lives on the engine, as the plan terms do).  `forecast`: None -- the env's plan forecast is left as it is (none set: perfect foresight, an oracle
    bound) --, or a mode's name for all four traces ("persistence", "daily"), or a dict of `set_plan_forecast`'s arguments; it is set
    on the env before the first decision."""

    DO_NOTHING = (1, 1, 2)

    def __init__(self, n_candidates: int = 8, horizon: int = 8, seed: int = 0, reward_weights=(1.0, 1.0, 1.0), gamma: float = 1.0,
                 info_weights=None, forecast=None):
        if n_candidates < 1 or horizon < 1:
            raise ValueError("ShootingMPCAgent: n_candidates and horizon must be positive")
        self.n_candidates, self.horizon, self.seed = int(n_candidates), int(horizon), int(seed)
        self.reward_weights, self.gamma, self.info_weights = tuple(reward_weights), float(gamma), info_weights
        self.forecast = forecast
        self._gen = None
        self.last = None
        self.last_horizon = 0

    def act(self, env):
        """env: an SdcEngine or a SustainDCVecEnv -> int32 device tensor [N, 3] (the vec env: [N, n_agents], its agents' columns)."""
        import torch
        eng = getattr(env, "engine", env)
        K, nothing = _mpc_horizon(env, self.horizon)[0], _do_nothing(env, self.DO_NOTHING)
        if K == 0:
            self.last, self.last_horizon = None, 0
            return nothing
        if self._gen is None:
            if self.forecast is not None:
                _set_forecast(env, self.forecast)
            self._gen = torch.Generator(device=eng.device)
            self._gen.manual_seed(self.seed)
        cand = torch.randint(0, 3, (self.n_candidates, K) + tuple(nothing.shape), generator=self._gen, device=eng.device, dtype=torch.int32)
        cand[0] = nothing
        self.last, self.last_horizon = env.plan(cand, self.reward_weights, self.gamma, self.info_weights), K
        return self.last.action


class CEMMPCAgent:
    """Model-predictive control with the cross-entropy method, the simulator as its own model: at every decision run `n_iters`
    iterations of "sample `n_candidates` sequences of `horizon` steps per env from a per-step, per-agent categorical distribution, score
    them, refit the distribution to the `n_elite` best" on the device (SdcEngine.plan_cem / SustainDCVecEnv.plan_cem over sdc_plan_cem:
    one call, one mark) and play the first action of the best sequence found.  alpha, p_min: the refit's smoothing and probability
    floor; reward_weights, gamma, info_weights: the objective, as `plan` takes it.  Candidate 0 of every iteration is the incumbent --
    at first the do-nothing sequence (ls 1, dc 1, bat 2) -- so on the model the chosen sequence never scores below doing nothing.
    With `warm_start` the next decision starts from this one's result moved up by a step: best_seq[1:] with do-nothing appended, probs[1:]
    with a uniform last step (torch ops on the device); both start afresh when the episode step goes backwards (a reset) or the horizon
    grows.  The draws are keyed on (seed, the decision's number `draw`, which goes up by one per planned decision): two agents with one
    seed on twin envs choose the same actions.  The horizon is shortened to what the episode has left (the planner does not look across
    an episode's end); with fewer than two steps left the agent does nothing.  `last`: the latest CEMResult (None after a do-nothing
    fallback), `last_horizon` the horizon it used.  The agent plans through the env, so limits and a terminal term:
    `env.set_plan_terms`, a critic as the terminal value: `env.set_critic` + `env.set_plan_critic` (on the engine, like the terms: no
    argument here); `forecast` as ShootingMPCAgent's: set on the env before the first decision."""

    DO_NOTHING = (1, 1, 2)

    def __init__(self, n_candidates: int = 8, n_elite: int = 2, n_iters: int = 3, horizon: int = 8, seed: int = 0, alpha: float = 0.0,
                 p_min: float = 0.0, warm_start: bool = True, reward_weights=(1.0, 1.0, 1.0), gamma: float = 1.0, info_weights=None,
                 forecast=None):
        if n_candidates < 2 or not 1 <= n_elite <= n_candidates or n_iters < 1 or horizon < 1:
            raise ValueError("CEMMPCAgent: n_candidates >= 2, 1 <= n_elite <= n_candidates, n_iters and horizon positive")
        self.n_candidates, self.n_elite, self.n_iters, self.horizon = int(n_candidates), int(n_elite), int(n_iters), int(horizon)
        self.seed, self.alpha, self.p_min, self.warm_start = int(seed), float(alpha), float(p_min), bool(warm_start)
        self.reward_weights, self.gamma, self.info_weights = tuple(reward_weights), float(gamma), info_weights
        self.forecast = forecast
        self._forecast_set = forecast is None
        self.draw = 0
        self.last = None
        self.last_horizon = 0
        self._probs = self._best_seq = self._step = None

    @classmethod
    def shifted(cls, probs, best_seq, K):
        """(probs [k, N, 3, 3], best_seq [k, N, 3]) of one decision -> the next decision's, K <= k steps: moved up by a step, the
        last step uniform / do-nothing; new tensors on the same device"""
        import torch
        p = torch.full((K,) + tuple(probs.shape[1:]), 1.0 / 3.0, dtype=probs.dtype, device=probs.device)
        b = torch.tensor(cls.DO_NOTHING, dtype=best_seq.dtype, device=best_seq.device).expand((K,) + tuple(best_seq.shape[1:])).contiguous()
        p[:K - 1] = probs[1:K]
        b[:K - 1] = best_seq[1:K]
        return p, b

    def _start(self, step, K):
        """the (probs, best_seq) this decision starts from: the last decision's shifted, or (None, None) -- uniform and do-nothing --
        without warm start, on the first decision, after the episode step went backwards, and when the horizon has grown"""
        prev, self._step = self._step, step
        if not self.warm_start or self._probs is None or prev is None or step <= prev or K > self._probs.shape[0]:
            return None, None
        return self.shifted(self._probs, self._best_seq, K)

    def act(self, env):
        """env: an SdcEngine or a SustainDCVecEnv -> int32 device tensor [N, 3] (the vec env: [N, n_agents], its agents' columns)."""
        K, step = _mpc_horizon(env, self.horizon)
        if not self._forecast_set:
            _set_forecast(env, self.forecast)
            self._forecast_set = True
        self._before(env, step)
        if K == 0:
            self.last, self.last_horizon = None, 0
            self._probs = self._best_seq = None
            self._step = step
            return _do_nothing(env, self.DO_NOTHING)
        probs, best_seq = self._start(step, K)
        self.last = self._plan(env, K, probs=probs, best_seq=best_seq, seed=self.seed, draw=self.draw, alpha=self.alpha, p_min=self.p_min,
                               reward_weights=self.reward_weights, gamma=self.gamma, info_weights=self.info_weights)
        self.draw = (self.draw + 1) & 0xFFFFFFFF
        self.last_horizon = K
        self._probs, self._best_seq = self.last.probs, self.last.best_seq
        return self._chosen(self.last)

    def rollout_stats(self, env, n_steps, into=None):
        """n_steps decisions and steps in ONE library call (SdcEngine.rollout_cem_stats / SustainDCVecEnv.rollout_cem_stats) with this
        agent's parameters and carried state -> the call's EpisodeStats, its `plan` a PlanStats.  What n_steps rounds of `act(env)` and
        a step with its actions do, bit for bit; afterwards `draw`, the carried distribution, `last_horizon` and the step it was made
        at are what those rounds would have left, so `act()` may follow (`last` is None: the call keeps the last decision's arrays in
        the result's `mpc`, not a CEMResult).  `into`: an EpisodeStats of the env's to continue.  The engine's arguments are checked
        first: a refused call leaves the agent as it was, but for a `forecast`, which is set on the env before the first decision."""
        import torch
        eng = getattr(env, "engine", env)
        n_steps = int(n_steps)
        step = _mpc_horizon(env, self.horizon)[1]
        if not self._forecast_set:
            _set_forecast(env, self.forecast)
            self._forecast_set = True
        H, lead = self.horizon, self._lead(eng)
        sync = self._sync_due(step)
        # the carried result, if the first decision may start from it (_start's rule but for the horizon, which the library checks)
        carried = not sync and self.warm_start and self._probs is not None and self._step is not None and step > self._step
        probs = torch.empty((H, lead, 3, 3), dtype=torch.float64, device=eng.device)
        best_seq = torch.empty((H, lead, 3), dtype=torch.int32, device=eng.device)
        k = int(self._probs.shape[0]) if carried else 0
        if k:
            probs[:k], best_seq[:k] = self._probs, self._best_seq
        res = self._rollout(env, n_steps, sync, probs=probs, best_seq=best_seq, resume_steps=k, warm_start=self.warm_start, seed=self.seed,
                            draw=self.draw, alpha=self.alpha, p_min=self.p_min, idle_action=self.DO_NOTHING,
                            reward_weights=self.reward_weights, gamma=self.gamma, info_weights=self.info_weights, into=into)
        if sync:
            self._synced()
        c = res.mpc
        self.draw = (self.draw + c.planned) & 0xFFFFFFFF
        self.last, self.last_horizon = None, c.steps
        self._probs, self._best_seq = (c.probs[:c.steps], c.best_seq[:c.steps]) if c.steps else (None, None)
        self._step = step + n_steps - 1
        return res

    # what GroupCEMMPCAgent does differently: in act(), then in rollout_stats()
    def _before(self, env, step):
        pass

    def _plan(self, env, K, **kw):
        return env.plan_cem(K, self.n_iters, self.n_candidates, self.n_elite, **kw)

    def _chosen(self, res):
        return res.action

    def _lead(self, eng):      # the carried arrays' leading dimension: a distribution per env
        return eng.n_envs

    def _sync_due(self, step):
        return False

    def _synced(self):
        pass

    def _rollout(self, env, n_steps, sync, **kw):
        return env.rollout_cem_stats(n_steps, self.horizon, self.n_iters, self.n_candidates, self.n_elite, **kw)


class GroupCEMMPCAgent(CEMMPCAgent):
    """CEMMPCAgent with the samples in env slots: the batch is groups of `group_size` = R consecutive envs that hold one state, every
    replica plays one sampled sequence per iteration, and the whole iteration is one rollout of the batch (SdcEngine.plan_cem_groups /
    SustainDCVecEnv.plan_cem_groups over sdc_plan_cem_groups) -- up to 1 024 samples per group and iteration.  The decision counter,
    the horizon cut at the episode's end and the warm start are CEMMPCAgent's, per group: probs [K, G, 3, 3], best_seq [K, G, 3].
    `act` returns `step_actions` -- the group's best first action for every replica --, so stepping with it keeps a group identical.
    Replicas draw their own resets (those are keyed on the global env index), so the agent makes every group a copy of its first env
    (`sync_groups`) on its first decision and whenever the episode step has gone backwards (a reset or auto-reset), and starts probs
    and best_seq afresh then.  `last`: the latest GroupCEMResult (None after a do-nothing fallback).  As for CEMMPCAgent, limits and a
    terminal term: `env.set_plan_terms`, a critic as the terminal value: `env.set_critic` + `env.set_plan_critic` (on the engine: no
    argument here), and `forecast` (a "values" forecast must be identical within a group)."""

    def __init__(self, group_size: int, n_elite: int = 2, n_iters: int = 3, horizon: int = 8, seed: int = 0, alpha: float = 0.0,
                 p_min: float = 0.0, warm_start: bool = True, reward_weights=(1.0, 1.0, 1.0), gamma: float = 1.0, info_weights=None,
                 forecast=None):
        if group_size < 2 or not 1 <= n_elite <= group_size or n_iters < 1 or horizon < 1:
            raise ValueError("GroupCEMMPCAgent: group_size >= 2, 1 <= n_elite <= group_size, n_iters and horizon positive")
        super().__init__(int(group_size), n_elite, n_iters, horizon, seed, alpha, p_min, warm_start, reward_weights, gamma, info_weights,
                         forecast)
        self.group_size = int(group_size)
        self.syncs = 0      # how often the groups have been re-synchronised

    def _before(self, env, step):
        if self._sync_due(step):
            env.sync_groups(self.group_size)
            self._synced()

    def _plan(self, env, K, **kw):
        return env.plan_cem_groups(self.group_size, K, self.n_iters, self.n_elite, **kw)

    def _chosen(self, res):
        return res.step_actions

    def rollout_stats(self, env, n_steps, into=None):
        """n_steps decisions and steps in ONE library call (SdcEngine.rollout_cem_groups_stats / SustainDCVecEnv.rollout_cem_groups_stats)
        with this agent's parameters and carried state -> the call's EpisodeStats, its `plan` a PlanStats per group with `diverged`.
        What n_steps rounds of `act(env)` and a step with its actions do, bit for bit: the call syncs the groups inside the library
        exactly when `act` would call `sync_groups` -- on the first decision, and when the episode step has gone backwards --, counts it
        in `syncs` and drops the carried result.  n_steps may reach the episode's end, not cross it: one call per episode.  Afterwards
        `draw`, the carried distribution, `last_horizon` and the step it was made at are what those rounds would have left, so `act()`
        may follow (`last` is None).  `into`: an EpisodeStats of the env's to continue.  The engine's arguments are checked first: a
        refused call leaves the agent as it was, but for a `forecast`, which is set on the env before the first decision."""
        return super().rollout_stats(env, n_steps, into)

    def _lead(self, eng):
        return eng.n_envs // self.group_size

    def _sync_due(self, step):      # the first decision, or a new episode: the replicas drew resets of their own
        return self._step is None or step < self._step

    def _synced(self):
        self.syncs += 1
        self._probs = self._best_seq = None

    def _rollout(self, env, n_steps, sync, **kw):
        return env.rollout_cem_groups_stats(n_steps, self.group_size, self.horizon, self.n_iters, self.n_elite, sync=sync, **kw)
