#!/usr/bin/env python3
"""Generate tests/golden/critic_grad/critic_grad.npz from the *imported* reference: every parameter's .grad after its VCritic.update
(cal_value_loss over a ValueNorm that update() itself advances, times value_loss_coef, differentiated by torch autograd in fp32) for
R = 67 share_obs rows, four networks -- tanh and relu, each with the feature LayerNorm on and off -- and two losses: the Huber loss with
value clipping, and the MSE loss without.  Nothing of the reference's sources is copied: the fixture holds the inputs and what the
reference left.

Per configuration c and loss l (keys "<c>_<l>_..."; c = tanh_fn1, tanh_fn0, relu_fn1, relu_fn0; l = huber_clip, mse):
  sd_<key>: the state_dict BEFORE update();  share_obs [R, 29], value_preds [R, 1], returns [R, 1];
  norm_mean, norm_var: the normaliser's running_mean_var() AFTER its update inside update() (what the loss normalised the returns with);
  grad_<key>: every parameter's .grad after update();  value_loss, critic_grad_norm (what update returned);  the margins below.
clip_param, huber_delta, value_loss_coef, max_grad_norm: the arguments.

The generator asserts what lets an fp64 restatement take the reference's fp32 branches: the norm is below max_grad_norm (the stored
gradients are unclipped), no |u - vp| lies within 1e-4 of clip, no |e| within 1e-4 of delta, |l(eo) - l(ec)| > 1e-6 wherever d is outside
the clip, no relu pre-activation within 1e-5 of zero -- and that both Huber regimes and both sides of the clip occur.
The stored predictions are drawn away from the clip; where a drawn return still puts an error within the margin of delta, the
next input seed is taken (input_seed records which).

Needs the reference checkout: SDC_REFERENCE=<path> python tests/golden/gen_critic_grad_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_actor_eval_golden as G      # noqa: E402  (the configurations and the network arguments are that generator's)

R, CONFIGS = 67, G.CONFIGS
CLIP, DELTA, COEF, MAX_NORM = 0.2, 1.0, 1.0, 10.0
LOSSES = {"huber_clip": (True, True), "mse": (False, False)}


def _args(activation, feature_norm, huber, clipped):
    return dict(G._args(activation, feature_norm), critic_epoch=5, critic_num_mini_batch=1, value_loss_coef=COEF, huber_delta=DELTA,
                use_clipped_value_loss=clipped, use_huber_loss=huber, critic_lr=5e-4, max_grad_norm=MAX_NORM)


class Margin(Exception):
    """a drawn input sits too close to one of the loss's branch points: the next input seed is tried"""


def need(ok, what, value):
    if not ok:
        raise Margin("%s = %.3e" % (what, value))


def one(VCritic, ValueNorm, Box, torch, ci, activation, feature_norm, loss_name, huber, clipped, input_seed, out):
    """one configuration and loss with the inputs of `input_seed`: its entries into `out`; Margin when an input is too close to a branch"""
    torch.manual_seed(5100 + ci)
    rng = np.random.default_rng(input_seed)
    algo = VCritic(_args(activation, feature_norm, huber, clipped), Box(low=-10.0, high=10.0, shape=(29,), dtype=np.float32))
    g = torch.Generator().manual_seed(5300 + ci)
    with torch.no_grad():      # trained-looking: every parameter random, the LayerNorms' gains around one
        for k, p in algo.critic.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.35 if p.dim() == 2 else 0.2))
            if p.dim() == 1 and ("feature_norm.weight" in k or k.endswith("fc.2.weight") or k.endswith("fc.5.weight")):
                p.add_(1.0)
        algo.critic.v_out.weight.mul_(0.5)
    sd = {k: v.detach().clone().numpy() for k, v in algo.critic.state_dict().items()}
    assert ("base.feature_norm.weight" in sd) == feature_norm
    share = rng.standard_normal((R, 29)).astype(np.float32)
    share[1::3, 20:] = 0.0
    rnn = np.zeros((R, 1, 64), dtype=np.float32)
    masks = np.ones((R, 1), dtype=np.float32)
    with torch.no_grad():
        u = algo.critic(share, rnn, masks)[0].numpy().astype(np.float64)      # [R, 1]
        base = algo.critic.base
        x = torch.from_numpy(share)
        if feature_norm:
            x = base.feature_norm(x)
        fc = base.mlp.fc
        z1 = fc[0](x)
        z2 = fc[3](fc[2](fc[1](z1)))
    # the stored predictions on both sides of the clip -- their distance from the network's output drawn away from the clip
    # itself --, some exactly the network's; the returns such that, normalised, the errors reach past delta on both sides
    far = rng.random((R, 1)) < 0.5
    gap = np.where(far, rng.uniform(CLIP + 0.03, 0.6, (R, 1)), rng.uniform(0.01, CLIP - 0.03, (R, 1)))
    vp = (u + gap * rng.choice([-1.0, 1.0], (R, 1))).astype(np.float32)
    vp[::11] = u[::11].astype(np.float32)
    returns = (40.0 + 12.0 * (u + 1.2 * rng.standard_normal((R, 1)))).astype(np.float32)
    norm = ValueNorm(1)
    value_loss, grad_norm = algo.update((share, rnn, vp, returns, masks), value_normalizer=norm)
    grad_norm = float(grad_norm)
    assert grad_norm < MAX_NORM, grad_norm                                    # (unclipped)
    mean, var = (t.detach().numpy().astype(np.float32) for t in norm.running_mean_var())
    t = ((returns.astype(np.float32) - mean) / np.sqrt(var)).astype(np.float64)
    d = u - vp.astype(np.float64)
    dc = np.clip(d, -CLIP, CLIP)
    eo, ec = t - u, t - (vp.astype(np.float64) + dc)
    lfn = (lambda e: np.where(np.abs(e) <= DELTA, e * e / 2, DELTA * (np.abs(e) - DELTA / 2))) if huber else (lambda e: e * e / 2)
    clip_margin = float(np.abs(np.abs(d) - CLIP).min())
    need(clip_margin > 1e-4, "clip_margin", clip_margin)
    delta_margin = float(min(np.abs(np.abs(eo) - DELTA).min(), np.abs(np.abs(ec) - DELTA).min()))
    need(not huber or delta_margin > 1e-4, "delta_margin", delta_margin)
    outside = np.abs(d) > CLIP
    max_margin = float(np.abs(lfn(eo) - lfn(ec))[outside].min())
    need(not clipped or max_margin > 1e-6, "max_margin", max_margin)
    relu_margin = float(min(z1.abs().min(), z2.abs().min()))
    need(activation != "relu" or relu_margin > 1e-5, "relu_margin", relu_margin)
    assert outside.sum() >= 10 and (~outside).sum() >= 10                      # both sides of the clip
    assert (np.abs(eo) > DELTA).sum() >= 10 and (np.abs(eo) <= DELTA).sum() >= 10      # both Huber regimes
    assert (lfn(ec) > lfn(eo)).sum() >= 5 and (lfn(ec) < lfn(eo)).sum() >= 5
    c = "%s_%s" % (G.name(activation, feature_norm), loss_name)
    for k, v in sd.items():
        out[f"{c}_sd_{k}"] = v
    for k, p in algo.critic.named_parameters():
        out[f"{c}_grad_{k}"] = p.grad.detach().clone().numpy()
        assert out[f"{c}_grad_{k}"].dtype == np.float32
    out.update({f"{c}_share_obs": share, f"{c}_value_preds": vp, f"{c}_returns": returns, f"{c}_norm_mean": mean, f"{c}_norm_var": var,
                f"{c}_value_loss": np.float32(value_loss.item()), f"{c}_critic_grad_norm": np.float64(grad_norm),
                f"{c}_clip_margin": np.float64(clip_margin), f"{c}_delta_margin": np.float64(delta_margin),
                f"{c}_max_margin": np.float64(max_margin), f"{c}_relu_margin": np.float64(relu_margin)})
    print(c, "input seed %d" % input_seed, "loss %.4f grad norm %.4f margins: clip %.2e delta %.2e max %.2e pre-activation %.2e" % (
        value_loss.item(), grad_norm, clip_margin, delta_margin, max_margin, relu_margin))
    out[f"{c}_input_seed"] = np.int64(input_seed)


def main():
    G._reference()
    import torch
    from harl.algorithms.critics.v_critic import VCritic
    from harl.common.valuenorm import ValueNorm
    from dc_rl_amd.spaces import Box
    out = dict(clip_param=np.float64(CLIP), huber_delta=np.float64(DELTA), value_loss_coef=np.float64(COEF), max_grad_norm=np.float64(MAX_NORM),
               configs=np.array([G.name(*c) for c in CONFIGS]), losses=np.array(list(LOSSES)))
    for ci, (activation, feature_norm) in enumerate(CONFIGS):
        for li, (loss_name, (huber, clipped)) in enumerate(LOSSES.items()):
            for attempt in range(20):      # (the first input seed whose draws keep the margins)
                try:
                    one(VCritic, ValueNorm, Box, torch, ci, activation, feature_norm, loss_name, huber, clipped,
                        5200 + 10 * ci + li + 100 * attempt, out)
                    break
                except Margin as m:
                    print(G.name(activation, feature_norm), loss_name, "attempt", attempt, m)
            else:
                sys.exit("no input seed kept the margins")
    os.makedirs(os.path.join(HERE, "critic_grad"), exist_ok=True)
    path = os.path.join(HERE, "critic_grad", "critic_grad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
