"""Tests-only restatement of the closed loop's POLICY HEAD (TEST INFRASTRUCTURE, never imported by the product): what
sdc_rollout_actor does between an env's three logits and the action that reaches its env step, as include/sustaindc_hip.h
states it at sdc_rollout_actor.

  * `uniforms`  -- the Philox block of one (env, episode step): counter (episode step, env_index_base + env, the env's episode number,
                   0xAC70), key (seed's low word, seed's high word); words x, y, z -> agent_ls, agent_dc, agent_bat;
                   u = (word >> 8) * 2^-24.  On tests/reset_ref.philox4x32_10 (pinned by Random123's known-answer vectors).
  * `draw_ref`  -- m = max l; e_i = exp2((l_i - m) log2 e); t = u ((e0 + e1) + e2); action = (t >= e0) + (t >= e0 + e1), in fp64 from
                   the device's own fp32 logits, and which cases are UNSURE: t within BAND * (e0 + e1 + e2) of a threshold.  The
                   device does the same in fp32 with the hardware exp2 (~1 ulp): for |l_i - m| <= MAX_GAP its t and thresholds are
                   within a few 2^-24 of these relative to the sum, far inside BAND = 1e-5; a sure case therefore has ONE answer.
  * `mode_ref`  -- the first maximum (np.argmax; torch.argmax's rule, what Categorical.mode() returns).
  * the engines, networks and constant-logit cases tests/test_gpu_actor_head.py and tests/test_actor_ref.py share.
"""
from __future__ import annotations

import itertools

import numpy as np

from tests.reset_ref import philox4x32_10

STREAM = 0xAC70              # the closed loop's stream constant (counter word 3)
LOG2E = 1.4426950408889634
BAND = 1e-5                  # |t - threshold| <= BAND * sum: unsure
MAX_GAP = 20.0               # the band's derivation holds for m - l_i <= 20
UNSURE_CAP = 1e-3            # share of unsure cases a test may have (expected: 2 thresholds x 2 BAND = 4e-5)
EPISODE_STEPS = 96
HIGH_SEED = (0x9E3779B9 << 32) | 7       # a seed whose high key word is live
BASE = 1000003                           # an env_index_base (odd, above 2^16)

# the two launch shapes: two full 16-env workgroups plus a part-filled one of the pair kernel; one full 32-env workgroup plus three
# wavefronts of the four-envs-per-wavefront kernel (DEBUG_QUAD = debug_flags bit the dispatch takes for "quad at any size")
SHAPES = [(40, False), (44, True)]


def uniforms(seed, env_index_base, episode, steps):
    """-> u [len(steps), N, 3 agents] float64 (exact: 24-bit integers times 2^-24).  episode [N]: the envs' episode numbers,
    steps [K]: episode steps."""
    episode = np.asarray(episode).astype(np.int64)
    env = int(env_index_base) + np.arange(len(episode), dtype=np.int64)
    steps = np.asarray(steps, dtype=np.int64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x, y, z, _ = philox4x32_10(steps[:, None], env[None, :], episode[None, :], STREAM, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack([(w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 for w in (x, y, z)], -1)


def draw_ref(logits, u):
    """logits [..., 3] (the device's fp32), u [...] -> (action [...] int64, unsure [...] bool), everything in fp64."""
    l = np.asarray(logits, dtype=np.float64)
    m = l.max(-1, keepdims=True)
    e = np.exp2((l - m) * LOG2E)
    s = (e[..., 0] + e[..., 1]) + e[..., 2]
    t = np.asarray(u, dtype=np.float64) * s
    th0, th1 = e[..., 0], e[..., 0] + e[..., 1]
    action = (t >= th0).astype(np.int64) + (t >= th1).astype(np.int64)
    unsure = (np.abs(t - th0) <= BAND * s) | (np.abs(t - th1) <= BAND * s)
    return action, unsure


def mode_ref(logits):
    return np.argmax(np.asarray(logits), axis=-1)


def max_gap(logits):
    l = np.asarray(logits, dtype=np.float64)
    return float((l.max(-1, keepdims=True) - l).max())


# ---- constant-logit networks: w3 = 0, so that the logits are b3 bit for bit --------------------------------------------------------
def order_patterns():
    """The 13 weak orderings of three values, as rank triples over {0, 1, 2} ((0,0,0), (1,1,0), (0,1,2), ...)."""
    pats = [p for p in itertools.product(range(3), repeat=3) if set(p) == set(range(max(p) + 1))]
    assert len(pats) == 13
    return pats


# the levels the ranks stand for: far apart, and ONE fp32 ulp apart (a compare that rounds, or works on differences, would see a tie)
TIE_LEVELS = [np.array([0.0, 1.0, 2.0], dtype=np.float32),
              np.array([-3.0, np.nextafter(np.float32(-3.0), np.float32(0)), np.nextafter(np.nextafter(np.float32(-3.0), np.float32(0)), np.float32(0))],
                       dtype=np.float32)]


def tie_b3():
    """[26][3] fp32: the 13 patterns at both sets of levels."""
    return [lv[list(p)] for lv in TIE_LEVELS for p in order_patterns()]


# degenerate and skewed distributions, one launch each: (b3 of agent_ls, agent_dc, agent_bat); every agent meets the two-sided and the
# skewed case, so each of the three Philox words is held to both thresholds
ALWAYS = {(0.0, -200.0, -200.0): 0, (-200.0, 0.0, -200.0): 1, (-200.0, -200.0, 0.0): 2}
HALVES = (0.0, -200.0, 0.0)        # never 1; 0 iff u < 0.5, exactly (e1 underflows to 0: t = 2 u against thresholds 1 and 1)
SKEWED = (0.0, -3.0, -6.0)
CONSTANT_LAUNCHES = [((0.0, -200.0, -200.0), (-200.0, 0.0, -200.0), (-200.0, -200.0, 0.0)),
                     (HALVES, SKEWED, (-6.0, 0.0, -3.0)),
                     (SKEWED, (-3.0, -6.0, 0.0), HALVES),
                     ((-6.0, -3.0, 0.0), HALVES, SKEWED)]
CONSTANT_K = 8                     # steps per launch
CONSTANT_SEED = 5


def constant_unsure_share(N, seed=CONSTANT_SEED, env_index_base=0, episode=1):
    """The unsure share of the band rule over the NON-degenerate agents of CONSTANT_LAUNCHES, from Philox alone (the launches follow
    each other from episode step 0 of episode `episode`): what tests/test_actor_ref.py holds to UNSURE_CAP on the CPU."""
    n_unsure = n = 0
    for i, b3s in enumerate(CONSTANT_LAUNCHES):
        u = uniforms(seed, env_index_base, np.full(N, episode), i * CONSTANT_K + np.arange(CONSTANT_K))
        for a, b3 in enumerate(b3s):
            if min(b3) < -MAX_GAP:
                continue
            _, unsure = draw_ref(np.broadcast_to(np.float32(b3), u.shape[:2] + (3,)), u[..., a])
            n_unsure += int(unsure.sum())
            n += unsure.size
    return n_unsure / n


# ---- networks and engines ----------------------------------------------------------------------------------------------------------
def torch_actor(seed, activation="tanh", logit_scale=0.5, feature_norm=True):
    """tests/test_gpu_actor.py's network (the reference's StochasticPolicy, every parameter random) with the last layer scaled so that
    the logits stay within MAX_GAP of their maximum; feature_norm False: built with use_feature_normalization off -- no
    base.feature_norm.* in the state_dict, the inputs go to the first Linear as they are."""
    import torch
    from tests.test_gpu_actor import _torch_actor
    m = _torch_actor(seed, activation)
    with torch.no_grad():
        m.act.action_out.linear.weight.mul_(logit_scale)
    if not feature_norm:
        m.base.feature_norm = torch.nn.Identity()
        assert not any(k.startswith("base.feature_norm") for k in m.state_dict())
    return m


def constant_actor(b3, activation="tanh", seed=900):
    """A network whose last layer's weights are zero: logits = b3 whatever the observations."""
    import torch
    m = torch_actor(seed, activation)
    with torch.no_grad():
        m.act.action_out.linear.weight.zero_()
        m.act.action_out.linear.bias.copy_(torch.as_tensor(np.asarray(b3, dtype=np.float32)))
    return m


def set_actors(eng, nets, activation="tanh"):
    for a in range(3):
        sd = dict(nets[a].state_dict())
        sd["activation"] = activation
        eng.set_actor(a, sd)


def engine(N, quad, seed=5, env_index_base=0, steps=EPISODE_STEPS):
    from dc_rl_amd import _lib as L
    from dc_rl_amd import dc_config, traces
    from dc_rl_amd.engine import SdcEngine
    tb = traces.synthetic_tables("ny", 0)
    p = dc_config.size_datacenter("dc_config.json", 1, 30.0)
    e = SdcEngine(N, episode_steps=steps, auto_reset=True, seed=seed, debug_flags=L.DEBUG_QUAD if quad else 0, env_index_base=env_index_base)
    e.set_tables(0, tb["W"], tb["C"], tb["T"], tb["WB"])
    e.set_dc_params(0, p)
    e.assign(0, 0, 174, 188)
    return e


def kernel_name(quad):
    return "sdc_rollout_actor_quad_kernel" if quad else "sdc_rollout_actor_kernel"


class Launch:
    """One rollout_actor launch and what the policy head's rule needs of the engine BEFORE it: the envs' episode numbers and the
    episode step (the batch is in lock-step)."""

    def __init__(self, eng, k, sample, quad):
        self.episode = eng.get_state("episode").copy()
        self.step0 = eng.episode_steps - eng.steps_to_episode_end()
        self.steps = self.step0 + np.arange(k)
        self.obs_before = eng.obs.clone()
        out = eng.rollout_actor(k, sample=sample, want_logits=True)
        assert eng.last_step_kernel() == kernel_name(quad)
        self.obs = out[0]
        self.actions = out[5].cpu().numpy()          # [k, N, 3]
        self.logits = out[6].cpu().numpy()           # [k, N, 3 agents, 3]
        assert np.isfinite(self.logits).all()
        assert self.actions.min() >= 0 and self.actions.max() <= 2
        self.u = uniforms(eng.seed, eng.config["env_index_base"], self.episode, self.steps) if sample else None

    def inputs(self):
        """the observations the k steps' actions were chosen from [k, N, 3, 26]"""
        import torch
        return torch.cat([self.obs_before[None], self.obs[:-1]], 0).cpu()


class Tally:
    """sure cases must match; the unsure ones are counted against UNSURE_CAP"""

    def __init__(self):
        self.unsure = self.n = 0

    def check(self, launch, agents=(0, 1, 2), u=None):
        u = launch.u if u is None else u
        for a in agents:
            lg = launch.logits[:, :, a, :]
            assert max_gap(lg) <= MAX_GAP, (a, max_gap(lg))
            ref, unsure = draw_ref(lg, u[..., a])
            sure = ~unsure
            got = launch.actions[:, :, a]
            bad = np.argwhere(sure & (got != ref))
            assert len(bad) == 0, "agent %d: %d of %d sure draws differ, first at (step, env) %s: device %d, restated %d" % (
                a, len(bad), int(sure.sum()), (int(launch.steps[bad[0][0]]), int(bad[0][1])), got[tuple(bad[0])], ref[tuple(bad[0])])
            self.unsure += int(unsure.sum())
            self.n += unsure.size

    def share(self):
        return self.unsure / max(self.n, 1)

    def close(self, what):
        print("%s: %d unsure of %d draws (share %.2e)" % (what, self.unsure, self.n, self.share()))
        assert self.n > 0 and self.share() <= UNSURE_CAP, (self.unsure, self.n)
