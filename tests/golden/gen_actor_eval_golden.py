#!/usr/bin/env python3
"""Generate tests/golden/actor_eval/actor_eval.npz from the *imported* reference: what its StochasticPolicy.evaluate_actions and its
HAPPO.update compute for R = 67 observation rows (four full 16-row tiles and three rows), for four networks -- tanh and relu, each with
the feature LayerNorm on and off.  Nothing of the reference's sources is copied: the fixture holds the inputs (the parameters, the rows,
the actions, old log-probabilities, advantages and a factor) and what the reference returned.

Per configuration c (keys "<c>_..."; c = tanh_fn1, tanh_fn0, relu_fn1, relu_fn0):
  the state_dict BEFORE update() (update computes its loss, then steps its optimiser), every parameter randomised so that it looks trained
  and the last layer scaled so that the logits stay within tests/actor_ref.MAX_GAP of their maximum;
  obs [R, 26]: rows of order one; every third row zero-padded to 14 live entries (as agent_dc's are), every third to 13 (agent_bat's);
  actions [R, 1]; old_log_probs [R, 1]; advantages [R, 1]; factor [R, 1];
  logits [R, 3] = act.action_out.linear(base(obs)); action_log_probs [R, 1], entropy_rows [R] and dist_entropy (their mean) from
  evaluate_actions; imp_weights [R, 1] and policy_loss from update().

Needs the reference checkout: SDC_REFERENCE=<path> python tests/golden/gen_actor_eval_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
R = 67
CONFIGS = [("tanh", True), ("tanh", False), ("relu", True), ("relu", False)]
CLIP = 0.2


def name(activation, feature_norm):
    return "%s_fn%d" % (activation, int(feature_norm))


def _reference():
    ref = os.environ.get("SDC_REFERENCE")
    if not ref or not os.path.isdir(ref):
        sys.exit("set SDC_REFERENCE to the reference checkout")
    for p in (ref, os.path.join(HERE, "_shims"), os.path.join(REPO, "tests", "aux", "harl_stubs")):
        sys.path.insert(0, p)
    sys.path.insert(0, REPO)
    from harl.algorithms.actors.happo import HAPPO
    return HAPPO


def _args(activation, feature_norm):
    return dict(hidden_sizes=[64, 64], activation_func=activation, use_feature_normalization=feature_norm, initialization_method="orthogonal_",
                gain=0.01, use_policy_active_masks=True, use_naive_recurrent_policy=False, use_recurrent_policy=False, recurrent_n=1,
                data_chunk_length=10, action_aggregation="prod", lr=5e-4, opti_eps=1e-5, weight_decay=0.0, clip_param=CLIP, ppo_epoch=5,
                actor_num_mini_batch=1, entropy_coef=0.01, use_max_grad_norm=True, max_grad_norm=10.0, std_x_coef=1.0, std_y_coef=0.5)


def _obs(rng):
    x = rng.standard_normal((R, 26)).astype(np.float32)
    x[1::3, 14:] = 0.0
    x[2::3, 13:] = 0.0
    return x


def main():
    HAPPO = _reference()
    import torch
    from dc_rl_amd.spaces import Box, Discrete
    from tests import actor_ref as AR
    out = dict(clip_param=np.float64(CLIP), configs=np.array([name(*c) for c in CONFIGS]))
    for ci, (activation, feature_norm) in enumerate(CONFIGS):
        torch.manual_seed(4100 + ci)
        rng = np.random.default_rng(4200 + ci)
        algo = HAPPO(_args(activation, feature_norm), Box(low=-2.0, high=2.0, shape=(26,), dtype=np.float32), Discrete(3))
        g = torch.Generator().manual_seed(4300 + ci)
        with torch.no_grad():      # trained-looking: every parameter random, the LayerNorms' gains around one
            for k, p in algo.actor.named_parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.35 if p.dim() == 2 else 0.2))
                if p.dim() == 1 and ("feature_norm.weight" in k or k.endswith("fc.2.weight") or k.endswith("fc.5.weight")):
                    p.add_(1.0)
            algo.actor.act.action_out.linear.weight.mul_(0.5)
        sd = {k: v.detach().clone().numpy() for k, v in algo.actor.state_dict().items()}
        assert ("base.feature_norm.weight" in sd) == feature_norm
        obs = _obs(rng)
        actions = rng.integers(0, 3, size=(R, 1)).astype(np.int64)
        rnn = np.zeros((R, 1, 64), dtype=np.float32)
        masks = np.ones((R, 1), dtype=np.float32)
        with torch.no_grad():
            logits = algo.actor.act.action_out.linear(algo.actor.base(torch.from_numpy(obs))).numpy()
            logp, dist_entropy, dist = algo.evaluate_actions(obs, rnn, actions, masks, None, masks)
            ent_rows = dist.entropy().numpy()
        assert AR.max_gap(logits) <= AR.MAX_GAP, AR.max_gap(logits)
        logp = logp.numpy()
        old = (logp + 0.15 * rng.standard_normal((R, 1))).astype(np.float32)
        old[::11] = logp[::11]                                   # (some rows with a ratio of exactly one)
        adv = rng.standard_normal((R, 1)).astype(np.float32)
        adv[5::13] = 0.0
        factor = np.exp(0.1 * rng.standard_normal((R, 1))).astype(np.float32)
        policy_loss, dist_entropy2, _, imp = algo.update((obs, rnn, actions, masks, masks, old, adv, None, factor))
        assert dist_entropy2.item() == dist_entropy.item()
        c = name(activation, feature_norm)
        for k, v in sd.items():
            out[f"{c}_sd_{k}"] = v
        out.update({f"{c}_obs": obs, f"{c}_actions": actions.astype(np.int32), f"{c}_old_log_probs": old, f"{c}_advantages": adv,
                    f"{c}_factor": factor, f"{c}_logits": logits, f"{c}_action_log_probs": logp,
                    f"{c}_entropy_rows": ent_rows.astype(np.float32), f"{c}_dist_entropy": np.float32(dist_entropy.item()),
                    f"{c}_imp_weights": imp.detach().numpy(), f"{c}_policy_loss": np.float32(policy_loss.item())})
        assert out[f"{c}_logits"].dtype == np.float32 and out[f"{c}_imp_weights"].dtype == np.float32
    os.makedirs(os.path.join(HERE, "actor_eval"), exist_ok=True)
    path = os.path.join(HERE, "actor_eval", "actor_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
