#!/usr/bin/env python3
"""Generate tests/golden/train/train.npz from the *imported* reference: what its own HAPPO.train (agent 0) and VCritic.train with a
ValueNorm leave -- their generators' shuffled mini-batches, losses, torch autograd, clip_grad_norm_, Adam and ValueNorm.update, all the
reference's -- after 2 epochs x 2 mini-batches over buffers filled with one stored batch of T = 10 steps of N = 40 envs, once as the
reference runs (fp32) and once with its modules and the ValueNorm cast to fp64.  torch.randperm is wrapped while the generators run,
so that every permutation drawn is recorded as data; the fp64 run replays the fp32 run's.  Nothing of the reference's sources is
copied: the fixture holds the inputs drawn here and what the reference left.

Keys:  T, N, epochs, num_mini_batch, beta, lr, opti_eps, weight_decay, max_grad_norm, entropy_coef, clip_param, huber_delta,
  value_loss_coef;
  obs [T, N, 26], share_obs [T, N, 29], actions [T, N] int32, old_log_probs [T, N], advantages [T, N], returns [T, N],
  value_preds [T, N] fp32: the stored batch (the factor is ones);
  actor_sd/<key>, critic_sd/<key>: the networks before, under the reference's state_dict keys;
  actor_perms, critic_perms [epochs, T N] int32: the permutations the generators drew, in order;
  actor_p32, actor_p64 [6391], critic_p32, critic_p64 [6459]: the parameters after train(), flat in the params structs' order;
  value_norm32 fp32, value_norm64 fp64 [epochs * num_mini_batch, 3]: running_mean, running_mean_sq, debiasing_term after every update;
  actor_info32 / actor_info64 [4]: train_info's policy_loss, dist_entropy, actor_grad_norm, ratio; critic_info32 / critic_info64 [2]:
  value_loss, critic_grad_norm.

Needs the reference checkout: SDC_REFERENCE=<path> python tests/golden/gen_train_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_actor_eval_golden as G      # noqa: E402  (the network arguments are that generator's)
import gen_critic_grad_golden as GC    # noqa: E402

T, N, EPOCHS, MINI = 10, 40, 2, 2
BETA = 0.99999


def flat(module, order):
    sd = module.state_dict()
    return np.concatenate([sd[k].detach().numpy().reshape(-1) for k in order if k in sd])


def dress(module, seed, torch, last):
    """trained-looking parameters: every one random, the LayerNorms' gains around one, the last layer halved"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in module.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.35 if p.dim() == 2 else 0.2))
            if p.dim() == 1 and ("feature_norm.weight" in k or k.endswith("fc.2.weight") or k.endswith("fc.5.weight")):
                p.add_(1.0)
        last(module).weight.mul_(0.5)


class Perms:
    """torch.randperm wrapped: records what it draws, or replays a record"""

    def __init__(self, torch, replay=None):
        self.torch, self.real, self.drawn, self.replay = torch, torch.randperm, [], None if replay is None else list(replay)

    def __enter__(self):
        def randperm(n, *a, **kw):
            p = self.real(n, *a, **kw) if self.replay is None else self.torch.from_numpy(self.replay.pop(0).astype(np.int64))
            assert p.numel() == n
            self.drawn.append(p.numpy().astype(np.int32))
            return p
        self.torch.randperm = randperm
        return self

    def __exit__(self, *exc):
        self.torch.randperm = self.real


def main():
    HAPPO = G._reference()
    import torch
    from harl.algorithms.critics.v_critic import VCritic
    from harl.common.buffers.on_policy_actor_buffer import OnPolicyActorBuffer
    from harl.common.buffers.on_policy_critic_buffer_ep import OnPolicyCriticBufferEP
    from harl.common.valuenorm import ValueNorm
    from dc_rl_amd.engine import _ACTOR_SD_KEYS, _CRITIC_SD_KEYS
    from dc_rl_amd.spaces import Box, Discrete
    a_args = dict(G._args("tanh", True), ppo_epoch=EPOCHS, actor_num_mini_batch=MINI)
    c_args = dict(GC._args("tanh", True, True, True), critic_epoch=EPOCHS, critic_num_mini_batch=MINI)
    buf_args = dict(episode_length=T, n_rollout_threads=N, hidden_sizes=[64, 64], recurrent_n=1, gamma=0.99, gae_lambda=0.95, use_gae=True,
                    use_proper_time_limits=True)
    obs_space, share_space, act_space = (Box(low=-2.0, high=2.0, shape=(26,), dtype=np.float32),
                                         Box(low=-10.0, high=10.0, shape=(29,), dtype=np.float32), Discrete(3))
    out = dict(T=np.int64(T), N=np.int64(N), epochs=np.int64(EPOCHS), num_mini_batch=np.int64(MINI), beta=np.float64(BETA),
               lr=np.float64(a_args["lr"]), opti_eps=np.float64(a_args["opti_eps"]), weight_decay=np.float64(a_args["weight_decay"]),
               max_grad_norm=np.float64(a_args["max_grad_norm"]), entropy_coef=np.float64(a_args["entropy_coef"]),
               clip_param=np.float64(G.CLIP), huber_delta=np.float64(GC.DELTA), value_loss_coef=np.float64(GC.COEF))
    assert (c_args["critic_lr"], c_args["opti_eps"], c_args["weight_decay"], c_args["max_grad_norm"]) == (
        a_args["lr"], a_args["opti_eps"], a_args["weight_decay"], a_args["max_grad_norm"])

    # ---- the stored batch
    rng = np.random.default_rng(7100)
    obs = rng.standard_normal((T, N, 26)).astype(np.float32)
    obs[:, 1::3, 14:] = 0.0
    share = rng.standard_normal((T, N, 29)).astype(np.float32)
    share[:, 1::3, 20:] = 0.0
    actions = rng.integers(0, 3, (T, N)).astype(np.int32)
    advantages = rng.standard_normal((T, N)).astype(np.float32)
    returns = (rng.standard_normal((T, N)) * 2.0 - 3.0).astype(np.float32)
    value_preds = (rng.standard_normal((T, N)) * 0.5).astype(np.float32)

    # ---- the actor: agent 0's HAPPO.train
    torch.manual_seed(7200)
    perms = None
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        algo = HAPPO(a_args, obs_space, act_space)
        if tag == "32":
            dress(algo.actor, 7300, torch, lambda m: m.act.action_out.linear)
            actor_sd = {k: v.detach().clone() for k, v in algo.actor.state_dict().items()}
            with torch.no_grad():      # the batch's own log-probabilities: those of the actions under the actor before (the ratio starts at 1)
                lp, _, _ = algo.actor.evaluate_actions(obs.reshape(-1, 26), np.zeros((T * N, 1, 64), np.float32), actions.reshape(-1, 1),
                                                       np.ones((T * N, 1), np.float32), None, np.ones((T * N, 1), np.float32))
            old_log_probs = lp.numpy().reshape(T, N).astype(np.float32)
        algo.actor.load_state_dict(actor_sd)
        if dt == torch.float64:
            algo.actor.double()
            algo.tpdv = dict(algo.tpdv, dtype=dt)
            algo.actor.tpdv = dict(algo.actor.tpdv, dtype=dt)
        buf = OnPolicyActorBuffer(buf_args, obs_space, act_space)
        buf.obs[:-1] = obs
        buf.actions[:] = actions[..., None]
        buf.action_log_probs[:] = old_log_probs[..., None]
        buf.update_factor(np.ones((T, N, 1), dtype=np.float32))
        with Perms(torch, perms) as rec:
            info = algo.train(buf, advantages[..., None].copy(), "EP")
        perms = rec.drawn
        assert len(perms) == EPOCHS
        p = flat(algo.actor, _ACTOR_SD_KEYS.values())
        assert p.shape == (6391,) and p.dtype == (np.float32 if dt == torch.float32 else np.float64)
        out["actor_p" + tag] = p
        out["actor_info" + tag] = np.array([float(info[k]) for k in ("policy_loss", "dist_entropy", "actor_grad_norm", "ratio")])
        print("actor", tag, info)
    out["actor_perms"] = np.stack(perms)
    out.update({"actor_sd/" + k: v.numpy() for k, v in actor_sd.items()})

    # ---- the critic: VCritic.train with a ValueNorm
    perms = None
    for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
        algo = VCritic(c_args, share_space)
        if tag == "32":
            dress(algo.critic, 7400, torch, lambda m: m.v_out)
            critic_sd = {k: v.detach().clone() for k, v in algo.critic.state_dict().items()}
        algo.critic.load_state_dict(critic_sd)
        norm = ValueNorm(1, beta=BETA)
        if dt == torch.float64:
            algo.critic.double()
            norm.double()
            algo.tpdv = dict(algo.tpdv, dtype=dt)
            algo.critic.tpdv = dict(algo.critic.tpdv, dtype=dt)
            norm.tpdv = dict(norm.tpdv, dtype=dt)
        states, real_update = [], norm.update

        def update(x, real_update=real_update, norm=norm, states=states):
            real_update(x)
            states.append([getattr(norm, k).detach().numpy().reshape(-1)[0] for k in ("running_mean", "running_mean_sq", "debiasing_term")])
        norm.update = update
        buf = OnPolicyCriticBufferEP(buf_args, share_space)
        buf.share_obs[:-1] = share
        buf.value_preds[:-1] = value_preds[..., None]
        buf.returns[:-1] = returns[..., None]
        with Perms(torch, perms) as rec:
            info = algo.train(buf, value_normalizer=norm)
        perms = rec.drawn
        assert len(perms) == EPOCHS and len(states) == EPOCHS * MINI
        p = flat(algo.critic, _CRITIC_SD_KEYS.values())
        assert p.shape == (6459,) and p.dtype == (np.float32 if dt == torch.float32 else np.float64)
        out["critic_p" + tag] = p
        out["value_norm" + tag] = np.array(states, dtype=np.float32 if dt == torch.float32 else np.float64)
        out["critic_info" + tag] = np.array([float(info[k]) for k in ("value_loss", "critic_grad_norm")])
        print("critic", tag, info, states[-1])
    out["critic_perms"] = np.stack(perms)
    out.update({"critic_sd/" + k: v.numpy() for k, v in critic_sd.items()})
    out.update(obs=obs, share_obs=share, actions=actions, old_log_probs=old_log_probs, advantages=advantages, returns=returns,
               value_preds=value_preds)

    os.makedirs(os.path.join(HERE, "train"), exist_ok=True)
    path = os.path.join(HERE, "train", "train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "optim", "optim.npz"))


if __name__ == "__main__":
    main()
