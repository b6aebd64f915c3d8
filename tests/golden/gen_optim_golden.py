#!/usr/bin/env python3
"""Generate tests/golden/optim/optim.npz from the *imported* reference: the parameters its own HAPPO.update and VCritic.update leave --
their loss, torch autograd, nn.utils.clip_grad_norm_ and torch.optim.Adam, all the reference's -- after each of three consecutive
updates on one small stored batch, once as the reference runs (fp32) and once with its modules (and the critic's ValueNorm) cast to
fp64.  Nothing of the reference's sources is copied: the fixture holds what the reference left.

THE INPUTS are those of the existing fixtures, which stay as they are and are not stored again: the actor's configuration tanh_fn1 of
tests/golden/actor_grad/actor_grad.npz (state_dict before, obs, actions, old_log_probs, advantages, factor; R = 67 rows) and the
critic's configuration tanh_fn0_huber_clip of tests/golden/critic_grad/critic_grad.npz (state_dict before, share_obs, value_preds,
returns) -- one network with the feature LayerNorm and one without.  (The relu configurations are left out: their pre-activations keep
their margin from zero for the stored parameters only, not after a step.)

Keys:  actor_config, critic_config, lr, opti_eps, weight_decay, max_grad_norm, entropy_coef, clip_param, huber_delta, value_loss_coef;
  actor_p32_<u>, actor_p64_<u> [6391] (fp32 / fp64): the parameters after update u = 1, 2, 3, flat in sdc_actor_params' order;
  actor_grad_norm32 [3]: what update returned;
  critic_p32_<u>, critic_p64_<u> [6401]: the critic's, flat in sdc_critic_params' order without the absent ln0 entries;
  critic_norm_mean [3], critic_norm_var [3] fp32: the ValueNorm's running_mean_var() after its update inside update u of the fp32
  run (what that update's loss normalised the returns with); critic_grad_norm32 [3].

Needs the reference checkout: SDC_REFERENCE=<path> python tests/golden/gen_optim_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_actor_eval_golden as G      # noqa: E402  (the network arguments are that generator's)
import gen_critic_grad_golden as GC    # noqa: E402

UPDATES = 3
ACTOR_CONFIG, CRITIC_CONFIG, CRITIC_LOSS = ("tanh", True), ("tanh", False), "huber_clip"


def flat(module, order):
    sd = module.state_dict()
    return np.concatenate([sd[k].detach().numpy().reshape(-1) for k in order if k in sd])


def main():
    HAPPO = G._reference()
    import torch
    from harl.algorithms.critics.v_critic import VCritic
    from harl.common.valuenorm import ValueNorm
    from dc_rl_amd.engine import _ACTOR_SD_KEYS, _CRITIC_SD_KEYS
    from dc_rl_amd.spaces import Box, Discrete
    from tests import actor_grad_ref as AG
    from tests import critic_grad_ref as CG
    a_args = G._args(*ACTOR_CONFIG)
    huber, clipped = GC.LOSSES[CRITIC_LOSS]
    c_args = GC._args(*CRITIC_CONFIG, huber, clipped)
    out = dict(actor_config=np.array(G.name(*ACTOR_CONFIG)), critic_config=np.array("%s_%s" % (G.name(*CRITIC_CONFIG), CRITIC_LOSS)),
               lr=np.float64(a_args["lr"]), opti_eps=np.float64(a_args["opti_eps"]), weight_decay=np.float64(a_args["weight_decay"]),
               max_grad_norm=np.float64(a_args["max_grad_norm"]), entropy_coef=np.float64(a_args["entropy_coef"]),
               clip_param=np.float64(G.CLIP), huber_delta=np.float64(GC.DELTA), value_loss_coef=np.float64(GC.COEF))
    assert (c_args["critic_lr"], c_args["opti_eps"], c_args["weight_decay"], c_args["max_grad_norm"]) == (
        a_args["lr"], a_args["opti_eps"], a_args["weight_decay"], a_args["max_grad_norm"])

    # ---- the actor
    c = AG.case(*ACTOR_CONFIG)
    R = c["obs"].shape[0]
    rnn, masks = np.zeros((R, 1, 64), dtype=np.float32), np.ones((R, 1), dtype=np.float32)
    for dt, tag in ((torch.float32, "p32"), (torch.float64, "p64")):
        algo = HAPPO(a_args, Box(low=-2.0, high=2.0, shape=(26,), dtype=np.float32), Discrete(3))
        algo.actor.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
        if dt == torch.float64:
            algo.actor.double()
            algo.tpdv = dict(algo.tpdv, dtype=dt)
            algo.actor.tpdv = dict(algo.actor.tpdv, dtype=dt)
        norms = []
        for u in range(1, UPDATES + 1):
            _, _, grad_norm, _ = algo.update((c["obs"], rnn, c["actions"].astype(np.int64), masks, masks, c["old_log_probs"], c["advantages"],
                                              None, c["factor"]))
            norms.append(float(grad_norm))
            p = flat(algo.actor, _ACTOR_SD_KEYS.values())
            assert p.shape == (AG.N_PARAMS,) and p.dtype == (np.float32 if dt == torch.float32 else np.float64)
            out["actor_%s_%d" % (tag, u)] = p
        if dt == torch.float32:
            out["actor_grad_norm32"] = np.array(norms)
        print("actor", tag, "grad norms", norms)

    # ---- the critic
    c = CG.case(*CRITIC_CONFIG, CRITIC_LOSS)
    R = c["share_obs"].shape[0]
    rnn, masks = np.zeros((R, 1, 64), dtype=np.float32), np.ones((R, 1), dtype=np.float32)
    for dt, tag in ((torch.float32, "p32"), (torch.float64, "p64")):
        algo = VCritic(c_args, Box(low=-10.0, high=10.0, shape=(29,), dtype=np.float32))
        algo.critic.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
        norm = ValueNorm(1)
        if dt == torch.float64:
            algo.critic.double()
            norm.double()
            algo.tpdv = dict(algo.tpdv, dtype=dt)
            algo.critic.tpdv = dict(algo.critic.tpdv, dtype=dt)
            norm.tpdv = dict(norm.tpdv, dtype=dt)
        norms, means, variances = [], [], []
        for u in range(1, UPDATES + 1):
            _, grad_norm = algo.update((c["share_obs"], rnn, c["value_preds"], c["returns"], masks), value_normalizer=norm)
            norms.append(float(grad_norm))
            mean, var = (t.detach().numpy().reshape(-1)[0] for t in norm.running_mean_var())
            means.append(mean)
            variances.append(var)
            p = flat(algo.critic, _CRITIC_SD_KEYS.values())
            assert p.shape == (CG.N_PARAMS - 58,) and p.dtype == (np.float32 if dt == torch.float32 else np.float64)
            out["critic_%s_%d" % (tag, u)] = p
        if dt == torch.float32:
            out["critic_grad_norm32"] = np.array(norms)
            out["critic_norm_mean"], out["critic_norm_var"] = np.array(means, np.float32), np.array(variances, np.float32)
        print("critic", tag, "grad norms", norms, "ValueNorm", means, variances)

    os.makedirs(os.path.join(HERE, "optim"), exist_ok=True)
    path = os.path.join(HERE, "optim", "optim.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "critic_grad", "critic_grad.npz"))


if __name__ == "__main__":
    main()
