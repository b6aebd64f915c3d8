"""Argument work of the Python binding (engine.py, vec_env.py, multi_device.py), each rule written once: index lists and pair
lists, device-tensor checks, the layout of a step's output block, the shapes of the state arrays, reset overrides, the horizon rules.
Pure: NumPy, torch and the constants of `_lib`; the library is never loaded and no GPU touched, so tests/test_engine_args.py holds
every refusal text without one.  The texts are the entry points' own -- callers hand in their name and words.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L


# ---------------------------------------------------------------------- index lists and pair lists
def int_ids(x, what, n=None):
    """an int32 array of env / row indices (a scalar stays 0-d); ValueError for anything else.  With `n` the indices are held to
    [0, n) in place of the int32 bound."""
    a = np.asarray(x.cpu() if hasattr(x, "cpu") else x)
    if a.dtype.kind not in "iu" and not (a.size == 0 and a.dtype.kind == "f"):
        raise ValueError(f"{what} must hold integers, got {a.dtype}")
    if a.ndim > 1:
        raise ValueError(f"{what} must be one-dimensional, got shape {a.shape}")
    if n is not None:
        if a.size and (a.min() < 0 or a.max() >= n):
            raise ValueError(f"{what} holds an env index outside [0, {n})")
    elif a.size and (int(a.min()) < -2 ** 31 or int(a.max()) >= 2 ** 31):
        raise ValueError(f"{what} holds a value outside int32")
    a = a.astype(np.int32)
    return a if a.ndim == 0 else np.ascontiguousarray(a)      # (np.ascontiguousarray would make a scalar one-dimensional)


def pairs(first, second, who, first_words, second_words):
    """two int_ids results as contiguous arrays of one length (a 0-d `first` broadcast); ValueError in the caller's words"""
    second = np.ascontiguousarray(second.reshape(-1))
    first = np.ascontiguousarray(np.broadcast_to(first, second.shape) if first.ndim == 0 else first)
    if first.shape != second.shape:
        raise ValueError(f"{who}: {first.shape[0]} {first_words} for {second.shape[0]} {second_words}")
    return first, second


def clone_pairs(src, dst, n_envs):
    """SdcEngine.clone_pairs: (src, dst)"""
    d = int_ids(dst, "clone_envs: dst", n_envs)
    return pairs(int_ids(src, "clone_envs: src", n_envs), d, "clone_envs", "sources", "destinations")


def restore_pairs(snap_envs, envs=None, rows=None):
    """SdcEngine.restore_pairs for a snapshot of envs `snap_envs`: (rows, envs)"""
    n = int(snap_envs.shape[0])
    d = snap_envs if envs is None else int_ids(envs, "restore: envs").reshape(-1)
    if rows is None:
        if envs is not None and d.shape[0] != n:
            raise ValueError(f"restore: {d.shape[0]} envs for {n} snapshot rows: say which rows go where (rows=)")
        r = np.arange(n, dtype=np.int32)
    else:
        r = int_ids(rows, "restore: rows")
    return pairs(r, d, "restore", "rows", "envs")


def group_sync_pairs(group_size, n, n_name):
    """sync_groups' clone pairs for `n` envs in groups of `group_size`: (src, dst), every env but a group's first and that first env;
    ValueError in sync_groups' words, with the caller's name `n_name` for its env count"""
    R = int(group_size)
    if R < 2 or R > n or n % R:
        raise ValueError(f"sync_groups: group_size = {R} must be at least 2 and divide {n_name} = {n}")
    e = np.arange(n, dtype=np.int32)
    dst = e[e % R != 0]
    return dst - dst % R, dst


# ---------------------------------------------------------------------- device tensors
ANY, SOME = None, "some"        # a shape pattern's entries: an int (exactly that), ANY size, SOME (at least 1)


def is_tensor(x, dtype, shape, device=None, cuda=True):
    """x is a contiguous torch tensor of `dtype` whose shape fits the pattern `shape`, on a GPU (`cuda`) and on `device` if given"""
    import torch
    return (isinstance(x, torch.Tensor) and x.dtype == dtype and (x.is_cuda or not cuda) and x.is_contiguous() and
            x.dim() == len(shape) and all(n >= 1 if want is SOME else want is ANY or n == want for n, want in zip(x.shape, shape)) and
            (device is None or x.device == device))


def device_tensor(x, who, name, dtype, shape, text=None, device=None, plural=False):
    """ValueError unless x is a contiguous CUDA tensor of `dtype` fitting the pattern `shape` (`text`: how the message shows it;
    default the pattern itself) -- and, where the engine's `device` is given, on it.  `who`: the entry point ("": no prefix)."""
    pre = f"{who}: " if who else ""
    if not is_tensor(x, dtype, shape):
        raise ValueError(f"{pre}{name} must be a contiguous {str(dtype).split('.')[-1]} CUDA tensor of shape {text or tuple(shape)}")
    if device is not None and x.device != device:
        raise ValueError(f"{pre}{name} {'are' if plural else 'is'} on {x.device}, this engine runs on {device}")


# ---------------------------------------------------------------------- the actors on stored rows, the PPO terms
def agent_slot(who, agent, name="agent"):
    """an agent slot 0 (ls), 1 (dc) or 2 (bat) as an int; ValueError in the caller's name for anything else"""
    if isinstance(agent, bool) or not isinstance(agent, (int, np.integer)) or not 0 <= int(agent) < L.N_AGENTS:
        raise ValueError(f"{who}: {name} = {agent!r} must be 0 (ls), 1 (dc) or 2 (bat)")
    return int(agent)


def agent_slots(who, agents):
    """`agents` as a tuple of distinct slots, at least one; ValueError in the caller's name"""
    try:
        out = tuple(agent_slot(who, a, "an entry of agents") for a in agents)
    except TypeError:
        raise ValueError(f"{who}: agents must be a sequence of agent slots") from None
    if not out or len(set(out)) != len(out):
        raise ValueError(f"{who}: agents = {tuple(agents)!r} must name at least one slot and none twice")
    return out


def actor_rows(who, obs, agent, per_agent=None, device=None):
    """actor_logits' `obs` -> (offset in floats, row stride in floats, rows, the logits' shape): a contiguous float32 CUDA tensor
    (..., 26) of dense rows -- offset 0, stride 26 --, or (..., 3, 26) of which agent `agent`'s rows are taken -- offset 26 * agent,
    stride 78.  `per_agent`: which of the two (None: the second where the last but one dimension is 3).  ValueError in the caller's name."""
    import torch
    D = L.OBS_PAD
    if not (isinstance(obs, torch.Tensor) and obs.dtype == torch.float32 and obs.is_cuda and obs.is_contiguous() and obs.dim() >= 1 and
            obs.shape[-1] == D and obs.numel() > 0):
        raise ValueError(f"{who}: obs must be a contiguous float32 CUDA tensor of shape (..., {D}) or (..., {L.N_AGENTS}, {D}), not empty")
    if device is not None and obs.device != device:
        raise ValueError(f"{who}: obs is on {obs.device}, this engine runs on {device}")
    three = obs.dim() >= 2 and obs.shape[-2] == L.N_AGENTS
    if per_agent is None:
        per_agent = three
    if per_agent and not three:
        raise ValueError(f"{who}: per_agent asks for obs of shape (..., {L.N_AGENTS}, {D}), got {tuple(obs.shape)}")
    if per_agent:
        lead = tuple(obs.shape[:-2])
        return D * agent, L.N_AGENTS * D, int(np.prod(lead, dtype=np.int64)), lead + (3,)
    lead = tuple(obs.shape[:-1])
    return 0, D, int(np.prod(lead, dtype=np.int64)), lead + (3,)


def actor_row_values(who, x, name, dtype, lead, agent, device=None):
    """actor_backward's per-row `actions` -> (offset, stride in elements): a contiguous `dtype` CUDA tensor of shape `lead` (dense:
    offset 0, stride 1) or `lead` + (3,), of which agent `agent`'s column is taken (offset agent, stride 3).  ValueError in the caller's
    name."""
    import torch
    kind = str(dtype).split(".")[-1]
    if not (isinstance(x, torch.Tensor) and x.dtype == dtype and x.is_cuda and x.is_contiguous() and
            tuple(x.shape) in (tuple(lead), tuple(lead) + (L.N_AGENTS,))):
        raise ValueError(f"{who}: {name} must be a contiguous {kind} CUDA tensor of shape {tuple(lead)} or {tuple(lead) + (L.N_AGENTS,)}")
    if device is not None and x.device != device:
        raise ValueError(f"{who}: {name} is on {x.device}, this engine runs on {device}")
    if tuple(x.shape) == tuple(lead):        # (lead = (..., 3) with a dense tensor of that shape: dense wins, as the shapes say)
        return 0, 1
    return agent, L.N_AGENTS


def finite_float(who, name, value):
    """`value` as a float; ValueError in the caller's name for what is no real number (the library refuses what is not finite)"""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{who}: {name} = {value!r} must be a number")
    return float(value)


# ---------------------------------------------------------------------- the critic's gradient
def share_rows(who, share_obs, device):
    """rows of share_obs: a contiguous float32 CUDA tensor (..., 29) on the engine's `device` -> the rows' shape (...); ValueError in the
    caller's name for anything else"""
    import torch
    if not (isinstance(share_obs, torch.Tensor) and share_obs.dtype == torch.float32 and share_obs.is_cuda and share_obs.is_contiguous() and
            share_obs.dim() >= 1 and share_obs.shape[-1] == L.SHARE_OBS_DIM):
        raise ValueError(f"{who}: share_obs must be a contiguous float32 CUDA tensor of shape (..., {L.SHARE_OBS_DIM})")
    if share_obs.device != device:
        raise ValueError(f"{who}: share_obs is on {share_obs.device}, this engine runs on {device}")
    return tuple(share_obs.shape[:-1])


def any_shape(who, x, name, dtype, device):
    """a contiguous CUDA tensor of `dtype` on the engine's `device`, of whatever shape -> that shape; ValueError in the caller's name"""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dtype == dtype and x.is_cuda and x.is_contiguous()):
        raise ValueError(f"{who}: {name} must be a contiguous {str(dtype).split('.')[-1]} CUDA tensor")
    if x.device != device:
        raise ValueError(f"{who}: {name} is on {x.device}, this engine runs on {device}")
    return tuple(x.shape)


# ---------------------------------------------------------------------- the optimiser step
def adam_struct(who, lr, betas, eps, weight_decay, max_grad_norm) -> L.SdcAdam:
    """the step's hyper-parameters as the library's struct (max_grad_norm None: +inf, no clipping); ValueError in the caller's name for
    what is no number or no pair of betas -- the ranges are the library's to refuse"""
    try:
        b1, b2 = betas
    except (TypeError, ValueError):
        raise ValueError(f"{who}: betas = {betas!r} must be a pair (beta1, beta2)") from None
    num = lambda name, v: finite_float(who, name, v)
    return L.SdcAdam(lr=num("lr", lr), beta1=num("beta1", b1), beta2=num("beta2", b2), eps=num("eps", eps),
                     weight_decay=num("weight_decay", weight_decay),
                     max_grad_norm=float("inf") if max_grad_norm is None else num("max_grad_norm", max_grad_norm))


def flat_grads(who, grads, n, device):
    """an ActorGrads / CriticGrads (anything with .flat) or a flat tensor -> the contiguous float32 CUDA tensor [n] on `device`"""
    import torch
    flat = getattr(grads, "flat", grads)
    device_tensor(flat, who, "grads", torch.float32, (n,), f"({n},)", device)
    return flat


def optim_which(who, which):
    """`which` network an optimiser state belongs to: an agent slot 0 .. 2 -> that int, "critic" -> None; ValueError for anything else"""
    if isinstance(which, str):
        if which != "critic":
            raise ValueError(f"{who}: which = {which!r} must be an agent slot 0 (ls), 1 (dc), 2 (bat) or 'critic'")
        return None
    return agent_slot(who, which, "which")


def optim_arrays(who, state, n):
    """load_optim_state's `state` -> (m, v as contiguous float32 arrays [n], L.SdcOptimState); ValueError / KeyError in the caller's name"""
    arrays = []
    for name in ("m", "v"):
        if name not in state:
            raise KeyError(f"{who}: the state holds no {name!r}")
        a = np.ascontiguousarray(state[name].detach().cpu().numpy() if hasattr(state[name], "detach") else state[name], dtype=np.float32)
        if a.shape != (n,):
            raise ValueError(f"{who}: {name} has shape {a.shape}, expected ({n},)")
        arrays.append(a)
    st = L.SdcOptimState(step=int(state.get("step", 0)), beta1_pow=float(state.get("beta1_pow", 1.0)),
                         beta2_pow=float(state.get("beta2_pow", 1.0)), skipped=int(state.get("skipped", 0)))
    return arrays[0], arrays[1], st


# ---------------------------------------------------------------------- train on the device: ValueNorm, mini-batches, the schedule
def value_norm_struct(who, value_norm):
    """set_value_norm's argument as the library's struct: None -> None (uninstall); a (mean, var) pair -> running_mean = mean,
    running_mean_sq = var + mean^2, debiasing_term = 1; an object or dict with running_mean, running_mean_sq and debiasing_term -> those
    three in fp32.  ValueError / KeyError in the caller's name."""
    if value_norm is None:
        return None
    f = np.float32
    num = lambda v: f(np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32).reshape(-1)[0])
    if isinstance(value_norm, (tuple, list)):
        if len(value_norm) != 2:
            raise ValueError(f"{who}: value_norm must be None, a (mean, var) pair, or hold running_mean, running_mean_sq and debiasing_term")
        mean, var = num(value_norm[0]), num(value_norm[1])
        return L.SdcValueNorm(float(mean), float(f(var + f(mean * mean))), 1.0)
    get = (lambda k: value_norm[k]) if isinstance(value_norm, dict) else (lambda k: getattr(value_norm, k))
    try:
        return L.SdcValueNorm(*(float(num(get(k))) for k in ("running_mean", "running_mean_sq", "debiasing_term")))
    except (KeyError, AttributeError):
        raise KeyError(f"{who}: value_norm holds no running_mean / running_mean_sq / debiasing_term") from None


# OnPolicyBatch's per-step fields as dword rows: name -> (dwords per row, dwords per agent column or 0, who reads it: "actor", "critic"
# or "book" -- the bookkeeping no update reads).  dones is uint8: no dword array, gathered by torch (SdcEngine.minibatch).
MINIBATCH_FIELDS = {
    "obs": (L.N_AGENTS * L.OBS_PAD, L.OBS_PAD, "actor"), "actions": (3, 1, "actor"), "logits": (9, 3, "actor"),
    "action_log_probs": (3, 1, "actor"), "entropy": (3, 1, "actor"), "advantages": (1, 0, "actor"),
    "share_obs": (L.SHARE_OBS_DIM, 0, "critic"), "values": (1, 0, "critic"), "value_preds": (1, 0, "critic"), "returns": (1, 0, "critic"),
    "rewards": (3, 0, "book"), "masks": (1, 0, "book"),
}


def minibatch_segments(agent=None, actors=True, critic=True):
    """the dword segments of one minibatch gather: [(field, offset in a row, dwords copied, dwords per row)] -- with `agent` only that
    column of the per-agent fields; without `actors` / `critic` not their fields; the bookkeeping fields only with both"""
    out = []
    for name, (row, col, group) in MINIBATCH_FIELDS.items():
        if (group == "actor" and not actors) or (group == "critic" and not critic) or (group == "book" and not (actors and critic)):
            continue
        if col and agent is not None:
            out.append((name, col * agent, col, row))
        else:
            out.append((name, 0, row, row))
    return out


def minibatch_rows(who, T, N, num_mini_batch):
    """rows per mini-batch when T steps of N envs are cut into `num_mini_batch` pieces: (T / num_mini_batch) N; ValueError when it does
    not divide T (the reference drops the remainder's rows; we refuse)"""
    if isinstance(num_mini_batch, bool) or not isinstance(num_mini_batch, (int, np.integer)) or num_mini_batch < 1:
        raise ValueError(f"{who}: num_mini_batch = {num_mini_batch!r} must be a positive integer")
    if T % int(num_mini_batch):
        raise ValueError(f"{who}: num_mini_batch = {num_mini_batch} does not divide the batch's {T} steps")
    return T // int(num_mini_batch) * N


def perm_stream_id(who: int, epoch: int) -> int:
    """happo_train's stream_id of one epoch's permutation: (who << 32) | epoch, who = the agent slot, 3 for the critic"""
    return (int(who) << 32) | int(epoch)


# ---------------------------------------------------------------------- the horizon of lookahead and plan
def check_horizon(who, K, left=None, auto_reset=False):
    """ValueError for a horizon a mark cannot hold and -- `left` = steps_to_episode_end() given -- one that would finish an episode"""
    if K > L.MARK_MAX_STEPS:
        raise ValueError(f"{who}: K = {K} is more than a mark holds (MARK_MAX_STEPS = {L.MARK_MAX_STEPS})")
    if left is not None and auto_reset and K >= left:
        raise ValueError(f"{who}: K = {K} steps would finish an episode ({left} steps left): the auto-reset kills the mark")
    if left is not None and K > left:
        raise ValueError(f"{who}: K = {K} steps would run past the end of an episode ({left} steps left)")


# ---------------------------------------------------------------------- the plan forecast
def forecast_modes(who, **channels):
    """set_plan_forecast's channel arguments (L.FORECAST_CHANNELS: a mode's name, its code, or None = "perfect") -> the four codes in
    the library's order; ValueError in the caller's name for an unknown channel, name or code"""
    unknown = sorted(set(channels) - set(L.FORECAST_CHANNELS))
    if unknown:
        raise ValueError(f"{who}: {unknown[0]!r} is not a forecast channel {L.FORECAST_CHANNELS}")
    modes = []
    for ch in L.FORECAST_CHANNELS:
        m = channels.get(ch)
        if m is None:
            m = L.FORECAST_PERFECT
        elif isinstance(m, str):
            if m not in L.FORECAST_MODES:
                raise ValueError(f"{who}: {ch} = {m!r} is not a forecast mode {tuple(L.FORECAST_MODES)}")
            m = L.FORECAST_MODES[m]
        elif isinstance(m, (int, np.integer)) and not isinstance(m, bool):
            m = int(m)        # (a code outside 0..3 is the library's to refuse)
        else:
            raise ValueError(f"{who}: {ch} must be a forecast mode's name {tuple(L.FORECAST_MODES)} or code, got {type(m).__name__}")
        modes.append(m)
    return modes


def forecast_mode_names(modes):
    """the four codes -> {channel: mode name}"""
    names = {v: k for k, v in L.FORECAST_MODES.items()}
    return {ch: names[int(m)] for ch, m in zip(L.FORECAST_CHANNELS, modes)}


def forecast_entries(who, n, left):
    """ValueError for a count of forecast entries the library would refuse (`left` = steps_to_episode_end())"""
    if not 1 <= n <= L.MARK_MAX_STEPS + 2:
        raise ValueError(f"{who}: n = {n} outside [1, MARK_MAX_STEPS + 2 = {L.MARK_MAX_STEPS + 2}]")
    if n > left + 2:
        raise ValueError(f"{who}: n = {n} entries reach past the end of an episode ({left} steps left: at most that + 2)")


# ---------------------------------------------------------------------- the step's output block
# the step's outputs are views of ONE device allocation (obs | share_obs | rew | info as floats, then done as bytes), so that a
# host-side consumer can fetch a whole step with a single device->host copy (`out_flat`)
_OUT_FLOATS = (("obs", (L.N_AGENTS, L.OBS_PAD)), ("share", (L.SHARE_OBS_DIM,)), ("rew", (L.N_AGENTS,)), ("info", (L.INFO_DIM,)))


def out_layout(n):
    """the block of `n` envs -> ([(name, dtype name, shape, offset in floats)] in memory order: obs, share, rew, info, done; bytes)"""
    blocks, o = [], 0
    for name, per_env in _OUT_FLOATS:
        blocks.append((name, "float32", (n,) + per_env, o))
        o += n * int(np.prod(per_env))
    return blocks + [("done", "uint8", (n,), o)], o * 4 + n


def out_views(flat, n):
    """{name: view} of a flat uint8 tensor (host or device) holding the block of `n` envs"""
    import torch
    blocks, _ = out_layout(n)
    fl = flat[:blocks[-1][3] * 4].view(torch.float32)
    views = {name: fl[o:o + int(np.prod(shape))].view(shape) for name, _, shape, o in blocks[:-1]}
    views["done"] = flat[blocks[-1][3] * 4:]
    return views


# ---------------------------------------------------------------------- state arrays (get_state / set_state)
# an env's scalars, one entry per env: name -> dtype
STATE_SCALARS = {
    **dict.fromkeys(("cursor", "t_rel", "day", "hourq", "q_popped", "q_cum", "q_head", "q_cum_hm1", "last_delta", "consecutive", "scale",
                     "hist_len", "hist_pos", "episode", "loc_id", "cfg_id", "day_lo", "day_hi", "hist_n"), np.int32),
    **dict.fromkeys(("q_cumT", "q_cumT_hm1", "fault", "order_stat_sticky"), np.uint32),
    **dict.fromkeys(("stpt", "bat_load", "ci_min", "ci_den", "t_min", "t_den", "hist_ref"), np.float64),
}
# name -> (dtype, shape): a string is one of the engine's sizes (n_envs, hist_stride, lw, queue_stride, hist_cap)
STATE_ARRAYS = {
    **{name: (dt, ("n_envs",)) for name, dt in STATE_SCALARS.items()},
    "hist": (np.float32, ("n_envs", "hist_stride")),
    "t_win": (np.float64, ("n_envs", "lw")), "wb_win": (np.float64, ("n_envs", "lw")),
    "qtab": (np.uint32, ("n_envs", "queue_stride", 2)),
    "qcum_t": (np.uint32, ("queue_stride", "n_envs")),      # (get_state only: the slot-major mirrors, where the batch has them)
    "hist_t": (np.uint32, ("hist_cap", "n_envs")),
    "record": (np.uint32, ("n_envs", 64)),
    "ep_return": (np.float64, ("n_envs", 3)),
    "header": (np.uint32, ("n_envs", L.HDR_DWORDS)),
    "qwin": (np.uint32, ("n_envs", L.QWIN, 4)),
}


def _shape(shape, sizes):
    return tuple(sizes[d] if isinstance(d, str) else d for d in shape)


def state_array(name, sizes):
    """a zeroed host array for state `name` of an engine with `sizes`; KeyError for an unknown name"""
    dt, shape = STATE_ARRAYS[name]
    return np.zeros(_shape(shape, sizes), dtype=dt)


# ---------------------------------------------------------------------- reset overrides
# kind -> the fields of sdc_reset_override it sets: (field, dtype, shape)
_PER_ENV_I32 = tuple((f, np.int32, ("n_envs",)) for f in ("day", "hour"))
RESET_OVERRIDES = {
    # the reference's own draws (day, hour, roll, the year's coherent-noise array): the device does the rest
    "noise": _PER_ENV_I32 + (("roll_days", np.int32, ("n_envs",)), ("noise", np.float64, ("n_envs", L.TABLE_LEN))),
    "windows": _PER_ENV_I32 + tuple((f, np.float64, ("n_envs",)) for f in ("ci_min", "ci_max", "t_min", "t_max")) +
               tuple((f, np.float64, ("n_envs", "lw")) for f in ("t_win", "wb_win")),
}


def reset_override(override, sizes):
    """reset's `override` dict -> {field: contiguous host array} (the kind with "noise" if that key is there); ValueError for a shape"""
    kind = "noise" if "noise" in override else "windows"
    arrays = {f: np.ascontiguousarray(override[f], dtype=dt) for f, dt, _ in RESET_OVERRIDES[kind]}
    bad = [len(shape) for f, _, shape in RESET_OVERRIDES[kind] if arrays[f].shape != _shape(shape, sizes)]
    N = sizes["n_envs"]
    if bad and kind == "noise":
        raise ValueError(f"noise injection: noise ({N}, {L.TABLE_LEN}), day / hour / roll_days ({N},)")
    if 1 in bad:
        raise ValueError("override scalars must have shape (n_envs,)")
    if bad:
        raise ValueError(f"override weather windows must have shape ({N}, {sizes['lw']})")
    return arrays
