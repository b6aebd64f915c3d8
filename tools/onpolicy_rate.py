"""Measurement: SdcEngine.collect(672) at 4 096 envs -- the rollouts, one critic launch, sdc_action_log_probs and sdc_gae -- against the
same batch built on the surface the engine had before it: rollout_actor(want_logits=True, want_values=True) per segment, the bootstrap
row's value, the log-probabilities as torch's log_softmax in fp64, and the restatement's backward loop (tests/onpolicy_ref.py) in
torch ops on the device, one small launch per operation and step.  ONE process; device events around each call, one warm-up of every
route, then the median, min and max of seven; the two new kernels also on their own, on the collected arrays.  One JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from tools.critic_rate import VALUE_NORM, critic_weights
from tools.mark_rate import timed3

REPS = 7
N, EP = 4096, 672
GAMMA, LAMBDA = 0.99, 0.95


def torch_batch(eng):
    """the batch on the earlier surface -> (returns, advantages, masks, log_probs, mean, std)"""
    obs0, share0 = eng.obs.clone(), eng.share_obs.clone()
    v0 = eng.critic_values(share0)
    rew, done, acts, logits, values = [], [], [], [], [v0[None]]
    k = 0
    while k < EP:
        K = min(EP - k, eng.steps_to_episode_end())
        o, s, r, d, _, a, l, v = eng.rollout_actor(K, sample=True, want_logits=True, want_values=True)
        rew.append(r), done.append(d), acts.append(a), logits.append(l), values.append(v)
        k += K
    rew, done, acts, logits, values = (torch.cat(x) for x in (rew, done, acts, logits, values))
    lp = torch.log_softmax(logits.double(), -1).gather(-1, acts.long()[..., None])[..., 0].float()
    masks = torch.ones_like(values)
    masks[1:] = 1.0 - done.float()
    g, c = np.float32(GAMMA), np.float32(GAMMA * LAMBDA)
    gae = torch.zeros_like(values[0])
    returns = torch.empty_like(values[:EP])
    r0 = rew[..., 0]
    for t in range(EP - 1, -1, -1):
        delta = (r0[t] + (values[t + 1] * float(g)) * masks[t + 1]) - values[t]
        gae = delta + (masks[t + 1] * float(c)) * gae
        returns[t] = gae + values[t]
    adv = returns - values[:EP]
    a64 = adv.double()
    return returns, adv, masks, lp, a64.mean(), a64.std(unbiased=False)


def main():
    eng, _, _ = bench.build_engine(N, EP, 0, seed=99, debug_flags=0)
    for a, w in enumerate(bench.actor_weights()):
        eng.set_actor(a, w)
    eng.set_critic(critic_weights(), VALUE_NORM, "tanh")
    eng.reset()
    b = eng.collect(EP, GAMMA, LAMBDA)          # (warm: the handle's buffers are allocated; every route runs one episode)
    torch_batch(eng)
    torch.cuda.synchronize()
    assert eng.steps_to_episode_end() == EP
    collect = timed3(lambda: eng.collect(EP, GAMMA, LAMBDA), REPS)
    base = timed3(lambda: torch_batch(eng), REPS)
    gae = timed3(lambda: eng.gae(b.rewards, b.dones, b.values, GAMMA, LAMBDA, want_value_preds=True), REPS)
    logp = timed3(lambda: eng.action_log_probs(b.actions, b.logits), REPS)
    rollouts = timed3(lambda: eng.rollout_actor(EP, sample=True, want_logits=True), REPS)
    print(json.dumps(dict(what="collect", n_envs=N, n_steps=EP, collect_ms=collect[0], collect_ms_range=collect[1:],
                          torch_route_ms=base[0], torch_route_ms_range=base[1:], speedup=base[0] / collect[0],
                          gae_ms=gae[0], gae_ms_range=gae[1:], gae_GBps=N * EP * 33.0 / gae[0] / 1e6,
                          action_log_probs_ms=logp[0], action_log_probs_ms_range=logp[1:], rollout_actor_ms=rollouts[0],
                          rollout_actor_ms_range=rollouts[1:])), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
