"""The vector-env boundary HARL runners call (`ShareVecEnv`, harl/envs/env_wrappers.py:53-165), backed by one
MI355X batch instead of one OS process per environment.

`SustainDCVecEnv(env_args, n_envs, ...)` presents N coupled SustainDC environments:
  reset() -> (obs [N,3,26] f32, share_obs [N,3,29] f32, available_actions [N,3,3])        (env_wrappers.py:275-280)
  step(actions [N,3,1] | [N,3]) -> (obs, share_obs, rews [N,3,1], dones [N,3] bool, infos, available_actions)
                                                                                          (env_wrappers.py:262-273)
with the reference's auto-reset semantics (env_wrappers.py:176-190): an env whose episode ends is reset inside
the same step call, the returned obs are the reset obs, and `infos[i][0]["original_obs" | "original_state" |
"original_avail_actions"]` hold the pre-reset values.

Outputs are NumPy arrays by default (what `ShareSubprocVecEnv` returns after `np.stack`); with
`return_torch=True` they are device tensors (views of the engine's buffers, valid until the next call) so that a
GPU policy never round-trips through the host.  `infos` is a lazy sequence: the N x 3 dicts of the reference are
materialised only for the entries a caller touches; an `infos` object read after its info block has been overwritten
raises (never another step's values), `snapshot_infos=True` gives every step's `infos` its own copy;
`accumulate_logger_sums()` / `read_logger_sums()` keep the logger's per-step sums
(harl/envs/sustaindc/sustaindc_logger.py:87-101) in a device-side accumulator that is read once per episode.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from collections.abc import Mapping, Sequence
from typing import List, Optional, Union

import numpy as np

from . import _args as A
from . import _lib as L
from . import dc_config, traces
from .engine import SdcEngine, group_sync_pairs
from .make_envs_pyenv import make_bat_fwd_env, make_dc_pyeplus_env, make_ls_env
from .spaces import Box, Discrete

AGENTS = ["agent_ls", "agent_dc", "agent_bat"]
OBS_DIMS = (26, 14, 13)

# the 10 info keys the SustainDC logger sums every step (sustaindc_logger.py:87-101)
LOGGER_KEYS = ["bat_total_energy_with_battery_KWh", "bat_CO2_footprint", "dc_water_usage",
               "ls_unasigned_day_load_left", "ls_tasks_in_queue", "ls_tasks_dropped", "dc_ITE_total_power_kW",
               "dc_CT_total_power_kW", "dc_Compressor_total_power_kW", "dc_HVAC_total_power_kW"]

DEFAULT_ENV_ARGS = {  # EnvConfig.DEFAULT_CONFIG (sustaindc_env.py:38-80)
    "agents": list(AGENTS), "location": "ny", "cintensity_file": "NYIS_NG_&_avgCI.csv",
    "weather_file": "USA_NY_New.York-Kennedy.epw", "workload_file": "Alibaba_CPU_Data_Hourly_1.csv",
    "datacenter_capacity_mw": 1, "timezone_shift": 0, "days_per_episode": 7, "max_bat_cap_Mw": 2,
    "dc_config_file": "dc_config.json", "individual_reward_weight": 0.8, "flexible_load": 0.1,
    "ls_reward": "default_ls_reward", "dc_reward": "default_dc_reward", "bat_reward": "default_bat_reward",
    "evaluation": False, "actions_are_logits": False,
}


class ShareVecEnv(ABC):
    """Abstract vectorised multi-agent env (same surface as harl/envs/env_wrappers.py:53)."""

    closed = False
    viewer = None
    metadata = {"render.modes": []}

    def __init__(self, num_envs, observation_space, share_observation_space, action_space):
        self.num_envs = num_envs
        self.observation_space = observation_space
        self.share_observation_space = share_observation_space
        self.action_space = action_space

    @abstractmethod
    def reset(self):
        pass

    @abstractmethod
    def step_async(self, actions):
        pass

    @abstractmethod
    def step_wait(self):
        pass

    def close_extras(self):
        pass

    def close(self):
        if self.closed:
            return
        self.close_extras()
        self.closed = True

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    @property
    def unwrapped(self):
        return self


class _FinalObs:
    """The `original_obs / original_state / original_avail_actions` entries of the envs that finished in a step
    (env_wrappers.py:176-190 puts them into agent 0's info), built per env on first access from one host copy of the
    step's pre-reset observations."""

    def __init__(self, final_obs: np.ndarray, done: np.ndarray, agent_idx, n_agents: int, concat: bool = False,
                 width: int = L.OBS_PAD):
        self._fo, self._done, self._idx, self._k, self._concat, self._w = final_obs, done, agent_idx, n_agents, concat, width
        self._made = {}

    def get(self, key, default=None):
        e, a = key
        if a != 0 or not self._done[e]:
            return default
        d = self._made.get(e)
        if d is None:
            fo = self._fo[e]
            # states[2][-1] of the PADDED obs: agent_bat's zero padding (harlsustaindc_env.py:25-26, :80)
            if self._concat:    # harlsustaindc_env.py:83-85: the trained agents' padded observations, concatenated
                raw = fo[self._idx][:, :self._w].reshape(-1)
            else:
                raw = np.concatenate([fo[0, :26], fo[1, 11:12], fo[1, 13:14], fo[2, 25:26]])
            d = self._made[e] = {"original_obs": fo[self._idx][:, :self._w].copy(),
                                 "original_state": np.repeat(raw[None, :], self._k, axis=0),
                                 "original_avail_actions": np.ones((self._k, 3), dtype=np.float32)}
        return d


def final_obs_of(env, final_obs, done):
    """the _FinalObs of a step of `env` (a vector env or one shard's): the host copy of its pre-reset observations, who finished"""
    return _FinalObs(final_obs, done, env._agent_idx, env.n_agents, env.share_concat, env.obs_width)


def sel(x, agent_idx):
    """the trained agents' rows of a [N, 3, ...] array (all of them in the usual three-agent case)"""
    return x if len(agent_idx) == 3 else x[:, agent_idx]


def sel_obs(obs, agent_idx, width):
    """... of the [N, 3, 26] observation block, cut to the widest trained agent's width"""
    o = sel(obs, agent_idx)
    return o if width == L.OBS_PAD else o[:, :, :width]


def share3_np(share, obs, agent_idx, width, concat):
    """NumPy outputs: the same shared vector for every trained agent, [N, n_agents, share_dim] (the layouts: SustainDCVecEnv._share3)"""
    if concat:
        share = sel_obs(obs, agent_idx, width).reshape(obs.shape[0], width * len(agent_idx))
    return np.broadcast_to(share[:, None, :], (share.shape[0], len(agent_idx), share.shape[1]))


def three_columns(actions, agent_idx, device):
    """actions [..., n_agents] in the trained agents' order -> the engine's contiguous int32 [..., 3] on its device; with an agent
    subset the other slots' columns are filled with 1 (they are played on the device and never read)"""
    import torch as t
    a = actions if actions.dtype == t.int32 and actions.device == device else actions.to(device=device, dtype=t.int32)
    if len(agent_idx) != 3:
        full = t.ones(tuple(a.shape[:-1]) + (3,), dtype=t.int32, device=device)
        full[..., agent_idx] = a
        a = full
    return a.contiguous()


def keyed_sums(keys, values):
    """{key: sum}: `values` are the sums of the keys that are info columns, in order; the others (constant 0 in the reference too) 0.0"""
    out = {k: 0.0 for k in keys}
    out.update({k: float(v) for k, v in zip([k for k in keys if k in L.INFO_IDX], values)})
    return out


_INFOS = L.load_infos()        # csrc/sdc_infos.c: InfoSeq (`infos`), InfoView (`infos[i][a]`) -- C types, see there
Mapping.register(_INFOS.InfoView)
Sequence.register(_INFOS.InfoRow)
_DERIVED_KEYS = ("ls_action", "bat_a_t", "isterminal")
_KEY_TEMPLATES = {}


def _base_keys(const_keys):
    """The keys of an info dict without extra entries, in iteration order, as ONE shared dict_keys object (a C-level `in`)."""
    t = _KEY_TEMPLATES.get(const_keys)
    if t is None:
        t = _KEY_TEMPLATES[const_keys] = dict.fromkeys(list(L.INFO_COLS) + ["ls_task_age_histogram"] + list(const_keys) +
                                                       list(_DERIVED_KEYS))
    return t.keys()


class _InfoSource:
    """What the views of one step read from: the step's [N, K] info block (fetched once, guarded), and the entries that are
    not a column of it.  Referenced by the C side (InfoCore); holds no reference back to the `infos` object."""

    __slots__ = ("_t", "_rows", "actions", "_act_version", "_act_host", "done", "const", "extra", "_owner", "_gen", "_valid_for",
                 "_keys")

    def __init__(self, info_tensor, actions, done, const, extra, owner, valid_for, keys):
        self._t = info_tensor
        self._rows = None
        self.actions = actions
        # the [N, 3] action tensor may be the caller's own (a GPU policy's output, taken without a copy): remember its
        # version so that an in-place overwrite is noticed instead of read as this step's actions
        self._act_version = getattr(actions, "_version", None)
        self._act_host = None
        self.done = done
        self.const = const
        self.extra = extra
        self._owner, self._gen, self._valid_for = owner, (owner._gen if owner is not None else 0), valid_for
        self._keys = keys

    def applied_actions(self):
        """[N, 3] host copy of the actions this step applied (read once, on first access)."""
        if self._act_host is None:
            a = self.actions
            if self._act_version is not None and a._version != self._act_version:
                raise RuntimeError("the action tensor passed to step() has been modified in place since; read "
                                   "infos[...]['ls_action'] before overwriting it, or pass step() a copy")
            self._act_host = a.detach().cpu().numpy().copy() if hasattr(a, "detach") else np.array(a)
        return self._act_host

    def rows(self):
        """The step's info block as ONE float32 [N, K] host array: one bulk conversion on first access."""
        if self._rows is None:
            # the block this object reads from is reused by later steps: never hand out another step's values
            if self._owner is not None and self._owner._gen - self._gen > self._valid_for:
                raise RuntimeError("these infos belong to an earlier step whose info block has been overwritten; read them "
                                   "before stepping again or construct the env with snapshot_infos=True")
            # (a copy: the pinned host buffers are reused two steps later)
            r = self._t.detach().cpu().numpy() if hasattr(self._t, "detach") else np.asarray(self._t)
            self._rows = np.array(r, dtype=np.float32, order="C", copy=True)
            self._owner = None
        return self._rows

    # ---- entries that are not a column of the block or a per-env constant (the C side asks for these) ----
    def _slow_get(self, env, agent, key):
        ex = self.extra.get((env, agent))
        if ex and key in ex:
            return ex[key]
        if key == "ls_task_age_histogram":
            j = L.INFO_IDX["ls_task_age_hist0"]
            return np.array(self.rows()[env, j:j + 5], dtype=np.float64)
        if key == "ls_action":
            return int(self.applied_actions()[env, 0])
        if key == "bat_a_t":
            return ("charge", "discharge", "idle")[int(self.rows()[env, L.INFO_IDX["bat_action"]])]
        if key == "isterminal":
            return bool(self.done[env])
        raise KeyError(key)

    def _has_extra(self, env, agent):
        return bool(self.extra.get((env, agent)))

    def _full_keys(self, env, agent):
        return list(self._keys) + list(self.extra.get((env, agent)) or ())


class LazyInfos(_INFOS.InfoSeq):
    """`infos` of a step: tuple[N] of list[3] of dict in the reference (env_wrappers.py:262-273); here a C sequence over one
    [N, K] array (csrc/sdc_infos.c): `infos[i]` is the env's cached row of per-agent views (a read-only sequence), `infos[i][a]` a read-only
    mapping whose `get` / `[]` / `in` / `keys()` run in C -- so the access pattern of an unchanged HARL runner
    (`infos[i][0].get(key, 0)` for 10 keys per env in sustaindc_logger.py:87-101, `"bad_transition" in info[0].keys()` per
    env in on_policy_base_runner.py:459-471) costs what it costs on plain dicts, without building N x 3 dicts per step."""

    def __init__(self, info_tensor, actions, done, const, extra, owner=None, valid_for=0, n_agents=3, keys=None):
        const = const if isinstance(const, list) else list(const)
        if keys is None:      # (the envs hand their own in: one lookup per env object, not per step)
            keys = _base_keys(tuple(const[0].keys()) if const else ())
        src = _InfoSource(info_tensor, actions, done, const, extra, owner, valid_for, keys)
        super().__init__(len(done), n_agents, L.INFO_IDX, keys, const, src, bool(extra))
        self._src = src

    actions = property(lambda self: self._src.actions)
    done = property(lambda self: self._src.done)
    const = property(lambda self: self._src.const)
    extra = property(lambda self: self._src.extra)

    def applied_actions(self):
        return self._src.applied_actions()

    def rows(self):
        return self._src.rows()


Sequence.register(LazyInfos)


_WARNED_SHARE_DEFAULT = False


def _merge_args(env_args: Optional[dict]) -> dict:
    a = dict(DEFAULT_ENV_ARGS)
    if env_args:
        a.update(env_args)
    L.reward_codes(a)   # NotImplementedError for a reward method the device does not run
    # options of the reference's HARL layer that change what the runner receives: never silently ignored.
    # nonoverlapping_shared_obs_space: harlsustaindc_env.py:53 reads it with .get(..., False) -- an absent key means the
    # CONCATENATED shared observation (3 x 26 floats, :83-85), True (the shipped YAML) the 29-float layout (:78-80).
    # (sustaindc_ptzoo.py:29 subscripts the key, so the reference itself raises KeyError when it is absent; the HARL
    # layer's default is the one taken here.)
    if "nonoverlapping_shared_obs_space" not in a:
        global _WARNED_SHARE_DEFAULT
        if not _WARNED_SHARE_DEFAULT:
            _WARNED_SHARE_DEFAULT = True
            import warnings
            warnings.warn("env_args has no 'nonoverlapping_shared_obs_space': taking the HARL layer's .get default (False = the "
                          "trained agents' padded observations concatenated, 78 floats for three agents); the reference's shipped "
                          "sustaindc.yaml sets True (the 29-float layout)", stacklevel=3)
    a["nonoverlapping_shared_obs_space"] = bool(a.get("nonoverlapping_shared_obs_space", False))
    if not a.get("partial_obs", True):
        raise NotImplementedError("Fully observable states are no longer supported. Please set 'partial_obs' to True.")
    # actions_are_logits: the reference stores the flag and never reads it (sustaindc_env.py:204-205): accepted, ignored
    unknown = [x for x in a["agents"] if x not in AGENTS]
    if unknown:
        raise ValueError(f"unknown agents {unknown}; the environment has {AGENTS}")
    if not a["agents"]:
        raise ValueError("at least one agent must be trained")
    return a


class SustainDCVecEnv(ShareVecEnv):
    def __init__(self, env_args: Union[dict, List[dict], None] = None, n_envs: int = 1, seed: int = 0,
                 months: Optional[Sequence[int]] = None, device: int = 0, return_torch: bool = False,
                 auto_reset: bool = True, data_root: Optional[str] = None, env_index_base: int = 0,
                 snapshot_infos: bool = False):
        # (what __deepcopy__ builds the copy from)
        self._init_args = dict(env_args=env_args, n_envs=n_envs, seed=seed, months=months, device=device, return_torch=return_torch,
                               auto_reset=auto_reset, data_root=data_root, env_index_base=env_index_base, snapshot_infos=snapshot_infos)
        per_env = [_merge_args(a) for a in env_args] if isinstance(env_args, (list, tuple)) else [_merge_args(env_args)] * n_envs
        if len(per_env) != n_envs:
            raise ValueError("env_args list must have n_envs entries")
        days = {a["days_per_episode"] for a in per_env}
        if len(days) != 1:
            raise ValueError("all envs of one batch must share days_per_episode")
        rcodes = {L.reward_codes(a) for a in per_env}
        if len(rcodes) != 1:
            raise ValueError("all envs of one batch must share ls_reward / dc_reward / bat_reward")
        self.reward_method = rcodes.pop()
        # A subset of agents (sustaindc_env.py:172-191, :623-655): the others are played by the reference's base
        # do-nothing agents -- on the device (sdc_config.policy = DO_NOTHING for their slots) -- and the surface carries
        # the trained agents only, in the reference's order.  (`_allow_agent_subset`: the single-env facade SustainDC
        # keeps the three-agent arrays and plays the base agents itself.)
        subsets = {tuple(x for x in AGENTS if x in a["agents"]) for a in per_env}
        if len(subsets) != 1:
            raise ValueError("all envs of one batch must train the same agents")
        full = bool(per_env[0].get("_allow_agent_subset"))
        share_modes = {a["nonoverlapping_shared_obs_space"] for a in per_env}
        if len(share_modes) != 1:
            raise ValueError("all envs of one batch must share nonoverlapping_shared_obs_space")
        self.share_concat = not share_modes.pop()
        self.agents = list(AGENTS) if full else list(subsets.pop())
        self._agent_idx = [AGENTS.index(x) for x in self.agents]
        self.n_agents = len(self.agents)
        self.policy = tuple(0 if (full or x in self.agents) else 1 for x in AGENTS)
        self.return_torch = return_torch
        self.episode_steps = int(days.pop()) * 96
        if months is None:
            months = [a.get("month", 0) if a.get("month") is not None else 0 for a in per_env]
        self.months = [int(m) for m in months]
        # unique trace sets and data-centre parameter sets
        loc_keys, cfg_keys, loc_id, cfg_id = [], [], [], []
        for a in per_env:
            lk = (a["location"].lower(), a["workload_file"], int(a["timezone_shift"]))
            ci_loc, _ = traces.obtain_paths(a["location"])
            ck = (a["dc_config_file"], float(a["datacenter_capacity_mw"]), ci_loc)
            if lk not in loc_keys:
                loc_keys.append(lk)
            if ck not in cfg_keys:
                cfg_keys.append(ck)
            loc_id.append(loc_keys.index(lk))
            cfg_id.append(cfg_keys.index(ck))
        self.tables = [traces.get_tables(lk[0], lk[1], lk[2], data_root=data_root) for lk in loc_keys]
        self.data_source = self.tables[0]["source"]
        # the same factory calls SustainDC.__init__ makes (sustaindc_env.py:148-160)
        self.ls_env = make_ls_env(month=self.months[0], n_vars_ci=8, n_vars_energy=0, n_vars_battery=0, queue_max_len=1000)
        self.dc_envs = [make_dc_pyeplus_env(month=self.months[0] + 1, location=ck[2], dc_config_file=ck[0],
                                            datacenter_capacity_mw=ck[1], max_bat_cap_Mw=per_env[0]["max_bat_cap_Mw"],
                                            use_ls_cpu_load=True, add_cpu_usage=False)[0] for ck in cfg_keys]
        self.dc_env = self.dc_envs[0]
        tot = self.dc_env.ranges["Facility Total Electricity Demand Rate(Whole Building)"]
        self.bat_env = make_bat_fwd_env(month=self.months[0], max_bat_cap_Mwh=self.dc_env.ranges["max_battery_energy_Mwh"],
                                        max_dc_pw_MW=tot[1] / 1e6, dcload_max=tot[1], dcload_min=tot[0], n_fwd_steps=8)
        self.bat_env.dcload_max = self.dc_env.power_ub_kW / 4   # sustaindc_env.py:158-160
        self.bat_env.dcload_min = self.dc_env.power_lb_kW / 4
        self.engine = SdcEngine(n_envs, episode_steps=self.episode_steps, device=device, n_locations=len(loc_keys),
                                n_dc_configs=len(cfg_keys), auto_reset=auto_reset, seed=seed, queue_max_len=1000,
                                reward_method=self.reward_method, env_index_base=env_index_base, policy=self.policy)
        for i, tb in enumerate(self.tables):
            self.engine.set_tables(i, tb["W"], tb["C"], tb["T"], tb["WB"])
        for i, e in enumerate(self.dc_envs):
            self.engine.set_dc_params(i, e.sized)
        init_day = np.array([traces.get_init_day(m) for m in self.months])
        self.engine.assign(np.array(loc_id), np.array(cfg_id), np.maximum(0, init_day - 7), np.minimum(364, init_day + 7))
        self._cfg_id = cfg_id
        self._loc_keys, self._cfg_keys = loc_keys, cfg_keys
        # per-env constant info entries (envs/dc_gym.py:224-227, envs/bat_env_fwd_view.py:118-121, carbon_ls.py:294-297)
        self._const = []
        for i in range(n_envs):
            e = self.dc_envs[cfg_id[i]]
            c = e.DC_Config
            self._const.append({
                "ls_queue_max_len": 1000, "ls_norm_load_left": 0, "ls_unasigned_day_load_left": 0, "ls_penalty_flag": 0,
                "ls_enforced": 0, "dc_power_lb_kW": e.power_lb_kW, "dc_power_ub_kW": e.power_ub_kW,
                "dc_CW_pump_power_kW": (c.CW_PRESSURE_DROP * c.CW_WATER_FLOW_RATE) / c.CW_PUMP_EFFICIENCY,
                "dc_CT_pump_power_kW": (c.CT_PRESSURE_DROP * c.CT_WATER_FLOW_RATE) / c.CT_PUMP_EFFICIENCY,
                "bat_max_bat_cap": e.sized["bat_capacity"], "bat_dcload_min": e.power_lb_kW / 4,
                "bat_dcload_max": e.power_ub_kW / 4,
            })
        self._info_keys = _base_keys(tuple(self._const[0].keys()))
        # HARL pads every agent to the widest space OF THE TRAINED AGENTS (harlsustaindc_env.py:25-26, :30-33: 26 whenever
        # agent_ls is trained, 14 for dc + bat, 13 for bat alone)
        self.obs_width = L.OBS_PAD if full else max(OBS_DIMS[i] for i in self._agent_idx)
        obs_space = [Box(low=-2.0, high=2.0, shape=(self.obs_width,), dtype=np.float32) for _ in self.agents]
        if self.share_concat:
            # sustaindc_ptzoo.py:32-44: max observation width x number of agents, Box(0, 1)
            self.share_dim = self.obs_width * len(self.agents)
            share_space = [Box(low=np.float32(0), high=np.float32(1), shape=(self.share_dim,), dtype=np.float32) for _ in self.agents]
        else:
            self.share_dim = L.SHARE_OBS_DIM
            share_space = [Box(low=-2.0, high=2.0, shape=(L.SHARE_OBS_DIM,), dtype=np.float32) for _ in self.agents]
        act_space = [Discrete(3) for _ in self.agents]
        ShareVecEnv.__init__(self, n_envs, obs_space, share_space, act_space)
        import torch
        self._torch = torch
        self._avail = torch.ones((n_envs, self.n_agents, 3), dtype=torch.float32, device=self.engine.device)
        self._avail_np = np.ones((n_envs, self.n_agents, 3), dtype=np.float32)
        self._idx_t = torch.as_tensor(self._agent_idx, device=self.engine.device)
        self._logger_acc = None
        self._actions = None
        self._need_reset = True
        self._host = None       # pinned host output buffers (NumPy outputs only)
        self._host_flip = 0
        self._no_done = np.zeros(n_envs, dtype=bool)
        self._gen = 0
        self._torch_views = None
        self.snapshot_infos = bool(snapshot_infos)
        self._act_pin = None    # pinned host staging of NumPy actions
        self._act_flip = 0

    # ------------------------------------------------------------------ helpers
    def _out(self, t):
        return t if self.return_torch else t.cpu().numpy()

    def _share3(self, share, obs=None):
        # the same shared vector for every trained agent (harlsustaindc_env.py:87 `repeat`): the 29-float layout the
        # kernel writes, or -- nonoverlapping_shared_obs_space False -- the concatenation of the trained agents' padded
        # observations (:83-85), which is a VIEW of the step's obs block (contiguous [N, 3, 26] -> [N, 78])
        if self.share_concat:
            o = self._sel_obs(obs)
            share = o.reshape(o.shape[0], self.share_dim)
        return share.unsqueeze(1).expand(-1, self.n_agents, -1)

    def _sel(self, x):
        return sel(x, self._agent_idx)

    def _sel_obs(self, obs):
        return sel_obs(obs, self._agent_idx, self.obs_width)

    def _ready(self, who):
        if self._need_reset:
            raise ValueError(f"{who}: call reset() first")

    def _reset_layout(self, obs, share):
        """(obs, share_obs, available_actions) for ALL envs as reset() returns them: the trained agents, either shared-observation layout"""
        return self._out(self._sel_obs(obs)), self._out(self._share3(share, obs)), (self._avail if self.return_torch else self._avail_np)

    def _host_entries_follow(self, src_rows, dst, const, cfg_id, months):
        """The host's per-env entries of envs `dst` become entries `src_rows` of const / cfg_id / months (this env's own lists: a clone;
        a snapshot's: a restore)."""
        # new lists, not writes into the old ones: the `infos` of earlier steps keep theirs (they describe those steps)
        new = list(self._const), list(self._cfg_id), list(self.months)
        for a, b in zip(src_rows.tolist(), dst.tolist()):
            new[0][b], new[1][b], new[2][b] = const[a], cfg_id[a], months[a]
        self._const, self._cfg_id, self.months = new

    def _log_step(self, info):
        if self._logger_acc is not None:      # device-side logger sums: one small reduction per step, no read-back
            self._logger_acc.add_(info[:, self._logger_idx].sum(0, dtype=self._torch.float64))
            self._logger_steps += 1

    def seed(self, seed: int):
        self.engine.set_seed(seed)

    # ------------------------------------------------------------------ ShareVecEnv API
    def reset(self):
        obs, share = self.engine.reset()
        self._need_reset = False
        return self._reset_layout(obs, share)

    def clone_envs(self, src, dst):
        """Env dst[k] becomes an exact copy of env src[k] (copy.deepcopy of the reference's SustainDC, on the device: SdcEngine.clone_envs;
        a scalar src is broadcast).  dst finishes src's current episode exactly and draws episodes of its own from its next reset on.
        Returns (obs, share_obs, available_actions) for ALL envs in reset()'s layout -- the trained agents, either shared-observation
        layout -- so a rollout loop can overwrite its observation buffers with them.  The host's per-env entries follow as well: the
        constant info entries of dst's `infos` (its data-centre config is now src's), its config and month.  ValueError for what the
        engine refuses."""
        self._ready("clone_envs")
        s, d = self.engine.clone_pairs(src, dst)
        obs, share = self.engine.clone_envs(s, d)
        self._host_entries_follow(s, d, self._const, self._cfg_id, self.months)
        return self._reset_layout(obs, share)

    def snapshot(self, envs=None):
        """The complete state of envs (default: all) in a device buffer (SdcEngine.snapshot), with the rows' host-side entries: their
        constant info entries, data-centre config and month.  Read-only: the run goes on as without it."""
        self._ready("snapshot")
        snap = self.engine.snapshot(envs)
        ids = snap.envs.tolist()
        snap.extra = {"const": [self._const[i] for i in ids], "cfg_id": [self._cfg_id[i] for i in ids],
                      "months": [self.months[i] for i in ids], "cfg_keys": self._cfg_keys, "loc_keys": self._loc_keys}
        return snap

    def restore(self, snap, envs=None, rows=None):
        """Env envs[k] becomes snapshot row rows[k] (SdcEngine.restore: by default every row goes back to the env it was taken from; a
        scalar `rows` is broadcast).  The host's per-env entries follow: dst's constant info entries, config and month are the row's.
        Returns (obs, share_obs, available_actions) for ALL envs in reset()'s layout.  The device-side logger accumulator
        (accumulate_logger_sums) is a sum over the batch, not env state: a restore leaves it alone.  ValueError for a snapshot of a vector
        env with other data-centre configs or trace sets, and for what the engine refuses."""
        self._ready("restore")
        x = snap.extra
        if x.get("cfg_keys") != self._cfg_keys or x.get("loc_keys") != self._loc_keys:
            raise ValueError("restore: the snapshot was not taken from a vector env with these data-centre configs and trace sets")
        r, d = self.engine.restore_pairs(snap, envs, rows)
        obs, share = self.engine.restore(snap, d, r)
        self._host_entries_follow(r, d, x["const"], x["cfg_id"], x["months"])
        return self._reset_layout(obs, share)

    def mark(self, envs=None, max_steps: int = 16):
        """Save what the next `max_steps` steps can change in envs (default: all) -- SdcEngine.mark: ~2.3 KB per env for 16 steps against
        a snapshot's ~146 KB.  Read-only: the run goes on as without it.  One live mark per env; a reset of the env (auto-reset
        included), a clone or restore into it kill the mark."""
        self._ready("mark")
        return self.engine.mark(envs, max_steps)

    def rewind(self, mark, envs=None):
        """Undo the steps taken since `mark` in its envs, or in a subset of them (SdcEngine.rewind).  Returns (obs, share_obs,
        available_actions) for ALL envs in reset()'s layout.  Actions handed to step_async and not yet stepped are dropped (they were
        chosen from observations that no longer stand).  The host's per-env entries (constant info entries, config, month) belong to
        the episode and do not change inside it; an `infos` object of an earlier step keeps describing that step.  The device-side
        logger accumulator (accumulate_logger_sums) is NOT rewound: it counts what was stepped, detours included.  ValueError for
        what the engine refuses."""
        self._ready("rewind")
        obs, share = self.engine.rewind(mark, envs)
        self._actions = None
        return self._reset_layout(obs, share)

    def plan(self, actions, reward_weights=(1.0, 1.0, 1.0), gamma: float = 1.0, info_weights=None):
        """Score M candidate action sequences of K steps, pick every env's best, and come back (SdcEngine.plan).  `actions`: an int
        tensor [M, K, num_envs, n_agents] in this env's agent order; with an agent subset the other slots' columns are filled with 1
        (they are played on the device and never read), as step_async does.  -> PlanResult whose `action` [num_envs, n_agents] holds
        the subset's columns, ready for step(); `returns` keeps all three slots.  The run goes on as if the call had not happened;
        actions handed to step_async stay; the envs' live mark is used up.  ValueError for what the engine refuses."""
        self._ready("plan")
        t = self._torch
        if not (isinstance(actions, t.Tensor) and actions.dim() == 4 and tuple(actions.shape[2:]) == (self.num_envs, self.n_agents)):
            raise ValueError(f"plan: actions must be a tensor of shape (M, K, {self.num_envs}, {self.n_agents})")
        res = self.engine.plan(self._three_columns(actions), reward_weights, gamma, info_weights)
        return self._subset_columns(res, "action")

    def set_plan_terms(self, limits=None, terminal=None):
        """Limits on info columns and a terminal term for every later plan / plan_cem / plan_cem_groups of this env
        (SdcEngine.set_plan_terms, which documents the arguments); no arguments clears them.  They stay across reset() and go to a
        copy.deepcopy of this env."""
        self.engine.set_plan_terms(limits, terminal)

    @property
    def plan_terms(self):
        """(limits, terminal) in force (SdcEngine.plan_terms)"""
        return self.engine.plan_terms

    def set_critic(self, params, value_norm=None, activation="tanh"):
        """The V critic for critic_values() and the planners' terminal value (SdcEngine.set_critic, which documents the arguments).
        It stays across reset() and goes to a copy.deepcopy of this env.  NotImplementedError in the concatenated shared-observation
        layout: a critic trained there sees the agents' observations side by side (78 inputs), not the engine's 29-entry share_obs."""
        if self.share_concat:
            raise NotImplementedError("set_critic: this env hands out the concatenated shared observation (78 inputs); the critic "
                                      "kernel runs over the engine's 29-entry share_obs rows")
        self.engine.set_critic(params, value_norm, activation)

    def critic_values(self, share_obs):
        """The critic's value of every row of a contiguous float32 device tensor [..., 29] -> [...] (SdcEngine.critic_values)"""
        return self.engine.critic_values(share_obs)

    def set_plan_critic(self, weight):
        """The critic as the terminal value of every later plan / plan_cem / plan_cem_groups of this env (SdcEngine.set_plan_critic);
        0 turns it off.  The weight stays across reset() and goes to a copy.deepcopy of this env."""
        self.engine.set_plan_critic(weight)

    @property
    def plan_critic(self):
        """the plan critic's weight in force (SdcEngine.plan_critic)"""
        return self.engine.plan_critic

    def set_plan_forecast(self, workload=None, carbon=None, temperature=None, wet_bulb=None, values=None):
        """What every later plan / plan_cem / plan_cem_groups of this env believes the traces ahead are (SdcEngine.set_plan_forecast,
        which documents the arguments); `set_plan_forecast(None)` or no arguments clears it.  It stays across reset() and goes to a
        copy.deepcopy of this env, `values` cloned."""
        self.engine.set_plan_forecast(workload, carbon, temperature, wet_bulb, values)

    @property
    def plan_forecast(self):
        """the forecast in force (SdcEngine.plan_forecast)"""
        return self.engine.plan_forecast

    def future_traces(self, n):
        """the true traces of the next steps, float64 [n, num_envs, 4] (SdcEngine.future_traces)"""
        self._ready("future_traces")
        return self.engine.future_traces(n)

    def forecast_traces(self, n):
        """what the forecast in force gives from the current state, float64 [n, num_envs, 4] (SdcEngine.forecast_traces)"""
        self._ready("forecast_traces")
        return self.engine.forecast_traces(n)

    def _three_columns(self, actions):
        """`three_columns` of actions [..., n_agents] in this env's agent order"""
        return three_columns(actions, self._agent_idx, self.engine.device)

    def _subset_columns(self, res, *fields):
        """a plan result whose `fields` [..., 3] are narrowed to this env's agent columns"""
        if self.n_agents != 3:
            for f in fields:
                setattr(res, f, getattr(res, f)[:, self._agent_idx].contiguous())
        return res

    def _subset_fixed(self, fixed_action):
        """fixed_action of a CEM call under this env's agent subset: the other slots carry 1 in every sampled candidate"""
        fixed = [-1, -1, -1] if fixed_action is None else [int(x) for x in fixed_action]
        return fixed if self.n_agents == 3 else [fixed[i] if i in self._agent_idx else 1 for i in range(3)]

    def plan_cem(self, horizon, n_iters, n_candidates, n_elite, *, probs=None, best_seq=None, fixed_action=None, **kw):
        """Plan with the cross-entropy method and come back (SdcEngine.plan_cem, which documents the arguments; `probs` [K, num_envs,
        3, 3] and `best_seq` [K, num_envs, 3] are the engine's, all three slots).  With an agent subset the other slots are not
        planned for: every sampled candidate carries 1 in their columns (what `plan` fills them with; they are played on the device
        and never read) and their probs stay as they are.  -> CEMResult whose `action` [num_envs, n_agents] holds the subset's
        columns, ready for step().  The run goes on as if the call had not happened; the envs' live mark is used up.  ValueError for
        what the engine refuses."""
        self._ready("plan_cem")
        res = self.engine.plan_cem(horizon, n_iters, n_candidates, n_elite, probs=probs, best_seq=best_seq,
                                   fixed_action=self._subset_fixed(fixed_action), **kw)
        return self._subset_columns(res, "action")

    def sync_groups(self, group_size):
        """Every group of `group_size` consecutive envs becomes a copy of its first env (SdcEngine.sync_groups, through this env's
        clone_envs, so the host's per-env entries follow).  Returns what clone_envs returns."""
        return self.clone_envs(*group_sync_pairs(group_size, self.num_envs, "num_envs"))

    def plan_cem_groups(self, group_size, horizon, n_iters, n_elite, *, probs=None, best_seq=None, fixed_action=None, **kw):
        """Plan with the cross-entropy method over replica groups and come back (SdcEngine.plan_cem_groups, which documents the
        arguments; `probs` [K, G, 3, 3] and `best_seq` [K, G, 3] are the engine's, all three slots).  With an agent subset the other
        slots are not planned for: every sampled replica carries 1 in their columns and their probs stay as they are, as in plan_cem.
        -> GroupCEMResult whose `action` [G, n_agents] and `step_actions` [num_envs, n_agents] hold the subset's columns, the latter
        ready for step().  The run goes on as if the call had not happened; the envs' live mark is used up.  ValueError for what the
        engine refuses."""
        self._ready("plan_cem_groups")
        res = self.engine.plan_cem_groups(group_size, horizon, n_iters, n_elite, probs=probs, best_seq=best_seq,
                                          fixed_action=self._subset_fixed(fixed_action), **kw)
        return self._subset_columns(res, "action", "step_actions")

    def _stats_actions(self, actions, K, what):
        """an action sequence [K, num_envs, n_agents] in this env's agent order -> the engine's [K, num_envs, 3] int32; None: the trained
        agents play the reference's base do-nothing actions (utils/base_agents.py: ls 1, dc 1, bat 2), as the other slots do on the device"""
        t = self._torch
        dev = self.engine.device
        if actions is None:
            if K is None:
                raise ValueError(f"{what}: actions=None needs n_steps")
            return t.tensor([1, 1, 2], dtype=t.int32, device=dev).expand(int(K), self.num_envs, 3).contiguous()
        if not (isinstance(actions, t.Tensor) and actions.dim() == 3 and tuple(actions.shape[1:]) == (self.num_envs, self.n_agents)):
            raise ValueError(f"{what}: actions must be a tensor of shape (K, {self.num_envs}, {self.n_agents})")
        return self._three_columns(actions)

    def rollout_stats(self, actions=None, n_steps=None, into=None):
        """K env-steps reduced on the device to per-env statistics (SdcEngine.rollout_stats, which documents the result).  `actions`: an
        int tensor [K, num_envs, n_agents] in this env's agent order; with an agent subset the other slots' columns are filled with 1
        (they are played on the device and never read), as step_async does.  None with n_steps: every trained agent plays the
        reference's base do-nothing action (ls 1, dc 1, bat 2) -- the baseline the other slots already play.  The envs move as under K
        calls of step(); actions handed to step_async and not yet stepped are dropped.  THE LOGGER ACCUMULATOR
        (accumulate_logger_sums) IS LEFT ALONE: it counts what went through step(), and these steps did not.  ValueError for what the
        engine refuses."""
        self._ready("rollout_stats")
        a = self._stats_actions(actions, n_steps, "rollout_stats")
        if n_steps is not None and int(n_steps) != int(a.shape[0]):
            raise ValueError("rollout_stats: n_steps does not match the action sequence")
        return self._stats_done(self.engine.rollout_stats(a, into=into))

    def set_actor(self, agent, params):
        """One agent's actor network for rollout_actor_stats / evaluate(actors=True) (SdcEngine.set_actor, which documents `params`).
        `agent`: a name ("agent_ls", "agent_dc", "agent_bat") or a slot 0..2.  The actors stay across reset() and go to a copy.deepcopy
        of this env.  ValueError when this env trains an agent subset: the closed-loop kernel needs all three actors."""
        if self.n_agents != 3:
            raise ValueError(f"set_actor: this env trains {self.agents}; the actors run inside the kernel for all three agents only")
        if isinstance(agent, str):
            if agent not in AGENTS:
                raise ValueError(f"set_actor: unknown agent {agent!r}; the environment has {AGENTS}")
            agent = AGENTS.index(agent)
        if int(agent) not in (0, 1, 2):
            raise ValueError(f"set_actor: agent slot {agent} outside 0 (agent_ls), 1 (agent_dc), 2 (agent_bat)")
        self.engine.set_actor(int(agent), params)

    def _stats_done(self, res):
        """what every statistics call leaves behind on the host: pending actions dropped, the info buffer holds another step"""
        self._actions = None
        self._gen += 1      # (the engine's info buffer now holds another step: `infos` objects that view it say so)
        return res

    def _planned_stats(self, who, synced, *args, **kw):
        """the engine's closed-loop planner call `who`, refused under an agent subset; `synced`: the group size it syncs with first, or None"""
        if self.n_agents != 3:
            raise ValueError(f"{who}: this env trains {self.agents}; the library steps with the planner's best_action for all "
                             "three agents, which is not what step() plays in the other slots' columns")
        self._ready(who)
        res = getattr(self.engine, who)(*args, **kw)
        if synced is not None:
            self._groups_synced(synced)
        return self._stats_done(res)

    def _groups_synced(self, group_size):      # (inside a library call: the host's per-env entries follow as after sync_groups)
        self._host_entries_follow(*group_sync_pairs(group_size, self.num_envs, "num_envs"), self._const, self._cfg_id, self.months)

    def rollout_actor_stats(self, n_steps, sample=False, into=None, policy_stats=True):
        """K env-steps played by the three actors (set_actor) inside the kernel, reduced on the device to an EpisodeStats with a
        PolicyStats (SdcEngine.rollout_actor_stats, which documents the arguments and the result).  The envs move as under K calls of
        step(); actions handed to step_async and not yet stepped are dropped; the logger accumulator (accumulate_logger_sums) is left
        alone, as by rollout_stats.  ValueError for what the engine refuses."""
        self._ready("rollout_actor_stats")
        return self._stats_done(self.engine.rollout_actor_stats(n_steps, sample=sample, into=into, policy_stats=policy_stats))

    def action_log_probs(self, actions, logits, want_entropy=True):
        """Log-probabilities and entropies of played actions from their logits, engine layout [T, num_envs, 3] / [T, num_envs, 3, 3]
        (SdcEngine.action_log_probs)"""
        return self.engine.action_log_probs(actions, logits, want_entropy)

    def actor_logits(self, agent, obs, per_agent=None):
        """One actor's logits for stored observation rows, (..., 26) or (..., 3, 26) -> (..., 3) (SdcEngine.actor_logits); the envs are
        not touched"""
        return self.engine.actor_logits(agent, obs, per_agent)

    def evaluate_actions(self, obs, actions, *args, **kw):
        """The actors over a stored batch, engine layout [T, num_envs, 3, 26] / [T, num_envs, 3] -> (logits, log_probs, entropy)
        (SdcEngine.evaluate_actions, which documents the arguments and the result)"""
        return self.engine.evaluate_actions(obs, actions, *args, **kw)

    def ppo_terms(self, agent, new_log_probs, old_log_probs, advantages, *args, **kw):
        """Importance ratio, clipped surrogate, HAPPO factor and their statistics for one agent (SdcEngine.ppo_terms, which documents
        the arguments and the PPOTerms)"""
        return self.engine.ppo_terms(agent, new_log_probs, old_log_probs, advantages, *args, **kw)

    def actor_update_terms(self, batch, agent, *args, **kw):
        """One agent's PPO terms over an OnPolicyBatch with the actor now set (SdcEngine.actor_update_terms)"""
        return self.engine.actor_update_terms(batch, agent, *args, **kw)

    def ppo_dlogp(self, agent, new_log_probs, old_log_probs, advantages, *args, **kw):
        """The PPO loss's derivative per stored log-probability for one agent (SdcEngine.ppo_dlogp, which documents the arguments)"""
        return self.engine.ppo_dlogp(agent, new_log_probs, old_log_probs, advantages, *args, **kw)

    def actor_backward(self, agent, obs, actions, dlogp, *args, **kw):
        """The gradient of one actor's loss with respect to its parameters over stored rows (SdcEngine.actor_backward) -> ActorGrads"""
        return self.engine.actor_backward(agent, obs, actions, dlogp, *args, **kw)

    def actor_grads(self, batch, agent, *args, **kw):
        """The gradient of the reference's actor loss for one agent of an OnPolicyBatch (SdcEngine.actor_grads) -> (ActorGrads, PPOTerms)"""
        return self.engine.actor_grads(batch, agent, *args, **kw)

    def critic_raw_values(self, share_obs):
        """The critic's own output for rows of share_obs, before its ValueNorm's scale and shift (SdcEngine.critic_raw_values)"""
        return self.engine.critic_raw_values(share_obs)

    def value_loss(self, raw_values, value_preds, returns, *args, **kw):
        """The reference's value loss per element and its derivative per raw value (SdcEngine.value_loss, which documents the
        arguments) -> ValueLossTerms"""
        return self.engine.value_loss(raw_values, value_preds, returns, *args, **kw)

    def critic_backward(self, share_obs, dvalue):
        """The gradient of sum(dvalue * raw) with respect to the critic's parameters over stored rows (SdcEngine.critic_backward)
        -> CriticGrads"""
        return self.engine.critic_backward(share_obs, dvalue)

    def critic_grads(self, batch, *args, **kw):
        """The gradient of the reference's critic loss for an OnPolicyBatch (SdcEngine.critic_grads) -> (CriticGrads, ValueLossTerms)"""
        return self.engine.critic_grads(batch, *args, **kw)

    def actor_adam_step(self, agent, grads, lr, **kw):
        """One Adam step with gradient-norm clipping over one agent's actor on the device (SdcEngine.actor_adam_step, which documents
        the arguments) -> the norm before clipping"""
        return self.engine.actor_adam_step(agent, grads, lr, **kw)

    def critic_adam_step(self, grads, lr, **kw):
        """One Adam step with gradient-norm clipping over the critic on the device (SdcEngine.critic_adam_step) -> the norm before clipping"""
        return self.engine.critic_adam_step(grads, lr, **kw)

    def actor_update(self, batch, agent, *args, **kw):
        """One whole update of an agent's actor over an OnPolicyBatch on the device (SdcEngine.actor_update) -> (PPOTerms, grad norm)"""
        return self.engine.actor_update(batch, agent, *args, **kw)

    def critic_update(self, batch, *args, **kw):
        """One whole update of the critic over an OnPolicyBatch on the device (SdcEngine.critic_update) -> (ValueLossTerms, grad norm)"""
        return self.engine.critic_update(batch, *args, **kw)

    def actor_state_dict(self, agent):
        """One agent's actor as the device holds it now, under the reference's keys (SdcEngine.actor_state_dict)"""
        return self.engine.actor_state_dict(agent)

    def critic_state_dict(self):
        """The critic as the device holds it now, under the reference's keys (SdcEngine.critic_state_dict)"""
        return self.engine.critic_state_dict()

    def optim_state(self, which):
        """The optimiser state of an agent slot or of "critic" (SdcEngine.optim_state)"""
        return self.engine.optim_state(which)

    def load_optim_state(self, which, state):
        """optim_state's dict back into a network's optimiser (SdcEngine.load_optim_state)"""
        self.engine.load_optim_state(which, state)

    def set_critic_value_norm(self, value_norm):
        """The critic's ValueNorm alone, stream-ordered (SdcEngine.set_critic_value_norm)"""
        self.engine.set_critic_value_norm(value_norm)

    def set_value_norm(self, value_norm):
        """A ValueNorm kept on the device, which the critic's scale and shift then follow; None uninstalls (SdcEngine.set_value_norm)"""
        self.engine.set_value_norm(value_norm)

    def value_norm_state(self):
        """The installed ValueNorm as the device holds it now (SdcEngine.value_norm_state)"""
        return self.engine.value_norm_state()

    def value_norm_update(self, returns, beta=0.99999):
        """ValueNorm.update(returns) on the device, stream-ordered (SdcEngine.value_norm_update)"""
        self.engine.value_norm_update(returns, beta)

    def permutation(self, n, seed, stream_id=0):
        """A keyed pseudo-random bijection of 0 .. n-1 as an int32 device tensor (SdcEngine.permutation)"""
        return self.engine.permutation(n, seed, stream_id)

    def minibatch(self, batch, indices, *args, **kw):
        """The rows `indices` of an OnPolicyBatch as a dense MiniBatch, one gather launch (SdcEngine.minibatch, which documents the
        arguments)"""
        return self.engine.minibatch(batch, indices, *args, **kw)

    def happo_train(self, batch, **kw):
        """The reference's OnPolicyHARunner.train() over one OnPolicyBatch on the device: shuffled mini-batches, the HAPPO factor,
        ValueNorm's running update (SdcEngine.happo_train, which documents the arguments) -> TrainInfo"""
        return self.engine.happo_train(batch, **kw)

    def gae(self, rew, done, values, *args, **kw):
        """Returns, advantages and masks of a collected rollout (SdcEngine.gae, which documents the arguments and the result)"""
        return self.engine.gae(rew, done, values, *args, **kw)

    def collect(self, n_steps, *args, **kw):
        """An on-policy training batch of n_steps env-steps played by the three actors (SdcEngine.collect, which documents the arguments
        and the OnPolicyBatch), in the engine's layout: all three agents.  The envs move as under n_steps calls of step(); actions
        handed to step_async and not yet stepped are dropped; the logger accumulator (accumulate_logger_sums) is left alone, as by
        rollout_stats.  ValueError for what the engine refuses."""
        self._ready("collect")
        return self._stats_done(self.engine.collect(n_steps, *args, **kw))

    def rollout_cem_stats(self, n_steps, horizon, n_iters, n_candidates, n_elite, **kw):
        """n_steps env-steps planned by the cross-entropy method inside the library, reduced on the device to an EpisodeStats with a
        PlanStats (SdcEngine.rollout_cem_stats, which documents the arguments and the result; `probs` / `best_seq` are the engine's,
        all three slots).  The envs move as under n_steps rounds of plan_cem() and step(); actions handed to step_async and not yet
        stepped are dropped; the logger accumulator (accumulate_logger_sums) is left alone, as by rollout_stats.  ValueError when
        this env trains an agent subset -- plan_cem + step() would play 1 in the other slots' columns, the library steps with the
        planner's best_action of all three: the two would differ --, and for what the engine refuses."""
        return self._planned_stats("rollout_cem_stats", None, n_steps, horizon, n_iters, n_candidates, n_elite, **kw)

    def rollout_cem_groups_stats(self, n_steps, group_size, horizon, n_iters, n_elite, *, sync=False, **kw):
        """n_steps env-steps planned by the cross-entropy method over replica groups inside the library, reduced on the device to an
        EpisodeStats with a PlanStats per group (SdcEngine.rollout_cem_groups_stats, which documents the arguments and the result;
        `probs` / `best_seq` are the engine's, all three slots).  The envs move as under n_steps rounds of plan_cem_groups() and
        step(); with `sync` the call begins as sync_groups(group_size) does, and the host's per-env entries follow as after it.  Actions
        handed to step_async and not yet stepped are dropped; the logger accumulator (accumulate_logger_sums) is left alone, as by
        rollout_stats.  ValueError when this env trains an agent subset, as for rollout_cem_stats, and for what the engine refuses."""
        return self._planned_stats("rollout_cem_groups_stats", group_size if sync else None, n_steps, group_size, horizon, n_iters, n_elite,
                                   sync=sync, **kw)

    def evaluate(self, n_episodes, actions=None, *, actors=False, sample=False, mpc=None):
        """`n_episodes` whole episodes of the batch from a reset (SdcEngine.evaluate) -> an EpisodeStats with a leading [E] dimension.
        `actions`: None (do-nothing baseline, see rollout_stats), an int tensor [episode_steps, num_envs, n_agents] replayed every
        episode, or a callable episode -> such a tensor.  `actors=True`: the three actors (set_actor) play, by their distributions'
        mode or -- `sample` -- a draw, and the result carries a PolicyStats; ValueError together with `actions`.  `mpc=agent`: a
        CEMMPCAgent plans every step inside the library (rollout_cem_stats), and the result carries a PlanStats; ValueError together
        with `actions` or `actors`, and when this env trains an agent subset.  A GroupCEMMPCAgent plans over replica groups
        (rollout_cem_groups_stats, one call per episode that syncs the groups first; the host's per-env entries follow as after
        sync_groups), and the PlanStats is per group with `diverged`.  The logger accumulator
        (accumulate_logger_sums) is left alone.  Afterwards the envs stand at the start of a fresh episode when auto_reset is on;
        otherwise call reset()."""
        steps = self.episode_steps
        if mpc is not None:
            if actors or actions is not None:
                raise ValueError("evaluate: mpc= plays the planner's own actions: give neither actions nor actors")
            if self.n_agents != 3:
                raise ValueError(f"evaluate: this env trains {self.agents}; mpc= needs all three agents (rollout_cem_stats)")
            synced = getattr(mpc, "syncs", 0)
            res = self.engine.evaluate(n_episodes, mpc=mpc)
            if getattr(mpc, "syncs", 0) != synced:      # a GroupCEMMPCAgent's calls synced the groups: the host's entries follow once
                self._groups_synced(mpc.group_size)
        elif actors:
            if actions is not None:
                raise ValueError("evaluate: actors=True plays the actors' own actions: give no actions")
            res = self.engine.evaluate(n_episodes, actors=True, sample=sample)
        else:
            fixed = None if callable(actions) else self._stats_actions(actions, steps, "evaluate")
            if fixed is not None and int(fixed.shape[0]) != steps:
                raise ValueError(f"evaluate: actions must hold episode_steps = {steps} steps, got {int(fixed.shape[0])}")
            res = self.engine.evaluate(n_episodes, (lambda e: self._stats_actions(actions(e), steps, "evaluate")) if fixed is None else fixed)
        self._need_reset = not self.engine.config["auto_reset"]
        return self._stats_done(res)

    def _take_state(self, src):
        """This env (built from src's constructor arguments, never stepped) becomes a copy of src: every env restored from a snapshot
        of src's, the seed and the host-side state copied.  src not reset yet: nothing to restore."""
        self.engine.set_seed(src.engine.seed)
        self.engine._set_plan_terms_struct(src.engine._plan_terms_struct())
        modes, values = src.engine._plan_forecast_state()
        self.engine._set_plan_forecast_state(modes, None if values is None else values.to(self.engine.device, copy=True))
        # (the networks as src's device holds them now -- stepped ones are read back -- and their optimisers' state with them)
        for slot, p in sorted(src.engine._host_actors().items()):      # (before the reset below: it fills the closed loop's observation copy)
            self.engine._set_actor_struct(slot, p)
            self.engine.load_optim_state(slot, src.engine.optim_state(slot))
        if src.engine._host_critic() is not None:
            self.engine._set_critic_struct(src.engine._critic)
            self.engine.load_optim_state("critic", src.engine.optim_state("critic"))      # (an installed ValueNorm travels with it)
            self.engine.set_plan_critic(src.engine.plan_critic)
        self.months, self._cfg_id, self._const = list(src.months), list(src._cfg_id), list(src._const)
        if not src._need_reset:
            self.engine.reset()            # (the library restores into envs that have been reset once; every env is overwritten)
            self._need_reset = False
            self.restore(src.snapshot().to(self.engine.device))
            self.engine.out_flat.copy_(src.engine.out_flat)      # (the last step's outputs as well)
            self.engine.final_obs.copy_(src.engine.final_obs)
        if src._logger_acc is not None:
            self._logger_keys, self._logger_idx = list(src._logger_keys), list(src._logger_idx)
            self._logger_acc = src._logger_acc.to(self.engine.device, copy=True)
            self._logger_steps = src._logger_steps

    def __deepcopy__(self, memo):
        """copy.deepcopy: a fresh vector env from the same constructor arguments, every env restored from a snapshot of this one --
        same global indices and seed, so the copy follows this env exactly, across resets, until the two are given different
        actions.  Before reset() a copy is just a fresh env."""
        import copy
        new = type(self)(**copy.deepcopy(self._init_args, memo))
        memo[id(self)] = new
        new._take_state(self)
        return new

    def step_async(self, actions):
        t = self._torch
        if not isinstance(actions, t.Tensor):
            # host actions: through a pinned int32 staging buffer, asynchronously.  Two buffers alternate, and each carries
            # an event recorded behind its host->device copy: the buffer is rewritten only once that copy has run (with
            # device-resident outputs nothing else makes the host wait for the stream, so a caller that does not read
            # results could otherwise run several steps ahead and overwrite actions that have not been copied yet)
            if self._act_pin is None:
                self._act_pin = [t.empty((self.num_envs, self.n_agents), dtype=t.int32, pin_memory=True) for _ in range(2)]
                self._act_evt = [t.cuda.Event(), t.cuda.Event()]
                self._act_rec = [False, False]
            self._act_flip ^= 1
            k = self._act_flip
            pin = self._act_pin[k]
            if self._act_rec[k]:
                self._act_evt[k].synchronize()
            pin.numpy()[...] = np.asarray(actions).reshape(self.num_envs, self.n_agents)
            actions = pin.to(self.engine.device, non_blocking=True)
            self._act_evt[k].record(t.cuda.current_stream(self.engine.device))
            self._act_rec[k] = True
        self._actions = self._three_columns(actions.reshape(self.num_envs, self.n_agents))

    def step_wait(self):
        if self._need_reset:
            raise RuntimeError("call reset() before step()")
        t = self._torch
        a = self._actions
        self._actions = None
        obs, share, rew, done, info = self.engine.step(a)
        if self.return_torch:
            # no host synchronisation on the device-resident path: which envs finished comes from the engine's host
            # mirror of the step counters (sdc_last_done)
            ld = self.engine.last_done()
            done_h = ld if ld is not None else self._no_done
        else:
            # NumPy outputs: ONE asynchronous copy of the step's outputs (one device allocation) into a pinned host buffer,
            # ONE synchronisation (two buffer sets alternate, so the arrays of a step stay valid until the step after next)
            hb = self._host_buffers()
            hb["flat"].copy_(self.engine.out_flat, non_blocking=True)     # the whole step in ONE device->host copy
            self._torch.cuda.current_stream(self.engine.device).synchronize()
            done_h = hb["done"].numpy().astype(bool)
        extra = {}
        if done_h.any():    # ONE host copy of the pre-reset observations; the per-env entries are built when read
            extra = final_obs_of(self, self.engine.final_obs.cpu().numpy(), done_h)
        # `infos` (lazy): reads the step's [N, 44] info block on first access -- from the pinned host copy made with the
        # other outputs (NumPy mode: valid for one more step), from the device otherwise.  An access after the block has
        # been overwritten RAISES instead of returning a later step's values; `snapshot_infos=True` makes every infos
        # object own a copy (the reference returns materialised dicts).
        self._gen += 1
        if self.return_torch:
            # device-resident path: a device clone only when asked for (snapshot_infos) or when an episode ended (the
            # runners read the final step's infos after the auto-reset); else a guarded view of the engine's buffer
            snap = self.snapshot_infos or bool(extra)
            infos = LazyInfos(info.clone() if snap else info, a, done_h, self._const, extra, None if snap else self, 0,
                              self.n_agents, self._info_keys)
        else:
            infos = LazyInfos(hb["info"], a, done_h, self._const, extra, self, 1, self.n_agents, self._info_keys)   # pinned double buffer: one more step
            if self.snapshot_infos:
                infos.rows()
        self._log_step(info)
        k = self.n_agents
        if self.return_torch:
            # the engine's output tensors are persistent, so the shaped views are too (uint8 0/1 -> bool is a reinterpret)
            # (an agent SUBSET selects rows by index -- a copy, not a view: obs, rew and the concatenated shared observation
            # are then rebuilt every step)
            v = self._torch_views
            if v is None:
                share_is_view = (not self.share_concat) or k == 3
                v = (self._share3(share, obs) if share_is_view else None, done.view(t.bool).unsqueeze(1).expand(-1, k),
                     (obs, rew.unsqueeze(-1)) if k == 3 else None)
                self._torch_views = v
            o, r = v[2] if v[2] is not None else (self._sel_obs(obs), self._sel(rew).unsqueeze(-1))
            sh = v[0] if v[0] is not None else self._share3(share, obs)
            return o, sh, r, v[1], infos, self._avail
        obs_h = hb["obs"].numpy()
        share3 = share3_np(hb["share"].numpy(), obs_h, self._agent_idx, self.obs_width, self.share_concat)
        return (self._sel_obs(obs_h), share3, self._sel(hb["rew"].numpy())[..., None],
                np.repeat(done_h[:, None], k, axis=1), infos, self._avail_np)

    def _launch_into(self, host):
        """One step enqueued, its outputs on their way into the caller's pinned host tensors (`host`: obs / share / rew / info
        / done slices of a larger block) -- nothing waited for.  For SustainDCMultiDeviceVecEnv: every device is given its
        work before any is waited on."""
        if self._need_reset:
            raise RuntimeError("call reset() before step()")
        a = self._actions
        self._actions = None
        e = self.engine
        e.step(a)
        for name, x in (("obs", e.obs), ("share", e.share_obs), ("rew", e.rew), ("info", e.info), ("done", e.done)):
            host[name].copy_(x, non_blocking=True)
        self._log_step(e.info)
        return a

    def _host_buffers(self):
        t = self._torch
        if self._host is None:
            e = self.engine
            self._host = []
            for _ in range(2):
                flat = t.empty(e.out_flat.shape, dtype=t.uint8, pin_memory=True)
                self._host.append(dict(A.out_views(flat, e.n_envs), flat=flat))
        self._host_flip ^= 1
        return self._host[self._host_flip]

    def accumulate_logger_sums(self, keys: Sequence[str] = LOGGER_KEYS, enable: bool = True):
        """Keep the SustainDC logger's per-step sums (harl/envs/sustaindc/sustaindc_logger.py:87-101: each key summed over
        the envs, every step) in a device-side accumulator: one small reduction per step on the stream, no host
        synchronisation; `read_logger_sums()` brings the totals over once per episode / log interval."""
        t = self._torch
        self._logger_keys = [k for k in keys]
        self._logger_idx = [L.INFO_IDX[k] for k in keys if k in L.INFO_IDX]
        self._logger_acc = t.zeros(len(self._logger_idx), dtype=t.float64, device=self.engine.device) if enable else None
        self._logger_steps = 0

    def read_logger_sums(self, reset: bool = True):
        """-> ({key: sum over envs and steps since the last read}, steps accumulated).  ONE device->host copy."""
        if self._logger_acc is None:
            raise RuntimeError("call accumulate_logger_sums() first")
        out = keyed_sums(self._logger_keys, self._logger_acc.cpu().numpy())
        n = self._logger_steps
        if reset:
            self._logger_acc.zero_()
            self._logger_steps = 0
        return out, n

    def info_sums(self, keys: Sequence[str] = LOGGER_KEYS):
        """Sum over envs of the given info columns for the last step, computed on the device."""
        idx = [L.INFO_IDX[k] for k in keys if k in L.INFO_IDX]
        return keyed_sums(keys, self.engine.info[:, idx].sum(0).cpu().numpy())

    def close_extras(self):
        self.engine.close()
