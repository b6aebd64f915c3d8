#!/usr/bin/env python3
"""Generate tests/golden/actor_grad/actor_grad.npz from the *imported* reference: every parameter's .grad after its HAPPO.update
(policy_loss - entropy_coef * dist_entropy, differentiated by torch autograd in fp32) for R = 67 observation rows and four networks --
tanh and relu, each with the feature LayerNorm on and off --, with the networks and the inputs of gen_actor_eval_golden.py (the same
seeds, drawn in the same order).  Nothing of the reference's sources is copied: the fixture holds the inputs and what the reference left.

Per configuration c (keys "<c>_..."; c = tanh_fn1, tanh_fn0, relu_fn1, relu_fn0):
  sd_<key>: the state_dict BEFORE update();  obs [R, 26], actions [R, 1] int32, old_log_probs, advantages, factor [R, 1];
  grad_<key>: every parameter's .grad after update();  actor_grad_norm (what update returned);  ratio_margin, relu_margin.
entropy_coef, clip_param, max_grad_norm: the arguments.

The generator asserts what lets an fp64 restatement take the reference's fp32 branches: the norm is below max_grad_norm (the stored
gradients are unclipped), no ratio lies within 1e-4 of 1 +- clip, no relu pre-activation within 1e-5 of zero.

Needs the reference checkout: SDC_REFERENCE=<path> python tests/golden/gen_actor_grad_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_actor_eval_golden as G      # noqa: E402  (the configurations, the arguments and the observation rows are that generator's)

R, CONFIGS, CLIP = G.R, G.CONFIGS, G.CLIP


def main():
    HAPPO = G._reference()
    import torch
    from dc_rl_amd.spaces import Box, Discrete
    out = dict(clip_param=np.float64(CLIP), configs=np.array([G.name(*c) for c in CONFIGS]))
    for ci, (activation, feature_norm) in enumerate(CONFIGS):
        args = G._args(activation, feature_norm)
        torch.manual_seed(4100 + ci)
        rng = np.random.default_rng(4200 + ci)
        algo = HAPPO(args, Box(low=-2.0, high=2.0, shape=(26,), dtype=np.float32), Discrete(3))
        g = torch.Generator().manual_seed(4300 + ci)
        with torch.no_grad():
            for k, p in algo.actor.named_parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.35 if p.dim() == 2 else 0.2))
                if p.dim() == 1 and ("feature_norm.weight" in k or k.endswith("fc.2.weight") or k.endswith("fc.5.weight")):
                    p.add_(1.0)
            algo.actor.act.action_out.linear.weight.mul_(0.5)
        sd = {k: v.detach().clone().numpy() for k, v in algo.actor.state_dict().items()}
        obs = G._obs(rng)
        actions = rng.integers(0, 3, size=(R, 1)).astype(np.int64)
        rnn = np.zeros((R, 1, 64), dtype=np.float32)
        masks = np.ones((R, 1), dtype=np.float32)
        with torch.no_grad():
            logp, _, _ = algo.evaluate_actions(obs, rnn, actions, masks, None, masks)
            base = algo.actor.base
            x = torch.from_numpy(obs)
            if feature_norm:
                x = base.feature_norm(x)
            fc = base.mlp.fc
            z1 = fc[0](x)
            z2 = fc[3](fc[2](fc[1](z1)))
        logp = logp.numpy()
        old = (logp + 0.15 * rng.standard_normal((R, 1))).astype(np.float32)
        old[::11] = logp[::11]
        adv = rng.standard_normal((R, 1)).astype(np.float32)
        adv[5::13] = 0.0
        factor = np.exp(0.1 * rng.standard_normal((R, 1))).astype(np.float32)
        _, _, grad_norm, imp = algo.update((obs, rnn, actions, masks, masks, old, adv, None, factor))
        grad_norm = float(grad_norm)
        assert grad_norm < args["max_grad_norm"], grad_norm                      # (unclipped)
        ratio = imp.detach().numpy().astype(np.float64)
        ratio_margin = float(np.minimum(np.abs(ratio - (1.0 - CLIP)), np.abs(ratio - (1.0 + CLIP))).min())
        assert ratio_margin > 1e-4, ratio_margin
        relu_margin = float(min(z1.abs().min(), z2.abs().min()))
        assert activation != "relu" or relu_margin > 1e-5, relu_margin
        c = G.name(activation, feature_norm)
        for k, v in sd.items():
            out[f"{c}_sd_{k}"] = v
        for k, p in algo.actor.named_parameters():
            out[f"{c}_grad_{k}"] = p.grad.detach().clone().numpy()
            assert out[f"{c}_grad_{k}"].dtype == np.float32
        out.update({f"{c}_obs": obs, f"{c}_actions": actions.astype(np.int32), f"{c}_old_log_probs": old, f"{c}_advantages": adv,
                    f"{c}_factor": factor, f"{c}_actor_grad_norm": np.float64(grad_norm), f"{c}_ratio_margin": np.float64(ratio_margin),
                    f"{c}_relu_margin": np.float64(relu_margin)})
        print(c, "grad norm %.4f ratio margin %.2e pre-activation margin %.2e" % (grad_norm, ratio_margin, relu_margin))
    out["entropy_coef"] = np.float64(G._args("tanh", True)["entropy_coef"])
    out["max_grad_norm"] = np.float64(G._args("tanh", True)["max_grad_norm"])
    os.makedirs(os.path.join(HERE, "actor_grad"), exist_ok=True)
    path = os.path.join(HERE, "actor_grad", "actor_grad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
