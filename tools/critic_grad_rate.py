"""Measurement: what a HAPPO / MAPPO trainer pays for one critic gradient over the share_obs rows it stored.
  * SdcEngine.critic_grads over [672, 4096] and [105, 4096] rows (critic_raw_values, value_loss with its statistics, critic_backward)
    against the same network as a torch fp32 eager module doing forward, the loss of harl/algorithms/critics/v_critic.py
    cal_value_loss (Huber, clipped, the returns normalised by a fixed ValueNorm) and backward on the same device;
  * the sdc_critic_backward call on its own (three launches: the gradient kernel, the fp64 sum of the partials, grad_sq), next to the
    gradient kernel's floor from the matrix instructions alone: 288 v_mfma_f32_16x16x4_f32 of 32 cycles per wavefront and 16 rows
    (forward 32 + 64; backward dY1 64, dW2 64, dW1 32, the feature LayerNorm's dX 32), ONE wavefront on each of four SIMDs of 256 CUs at
    2.4 GHz.
tools/actor_grad_rate.py's protocol: ONE process; device events around each call; after one warm-up of every route the median
[min, max] of nine, the two routes alternated.  One JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bench
from actor_eval_rate import N, alternated

MFMA_PER_PASS = 32 + 64 + 64 + 64 + 32 + 32
MFMA_FLOOR_ROWS_PER_S = 256 * 4 * 16 / (MFMA_PER_PASS * 32 / 2.4e9)
CLIP, DELTA = 0.2, 10.0
VALUE_NORM = (-3.0, 7.5 ** 2)      # (mean, var)


def critic_weights(seed=11):
    """random weights of the reference's VNet shape (LayerNorm(29)-64-64-1, tanh)"""
    r = np.random.default_rng(seed)
    return {"ln0_g": 1 + 0.1 * r.standard_normal(29), "ln0_b": 0.1 * r.standard_normal(29),
            "w1": r.standard_normal((64, 29)) * 0.3, "b1": 0.1 * r.standard_normal(64),
            "ln1_g": 1 + 0.1 * r.standard_normal(64), "ln1_b": 0.1 * r.standard_normal(64),
            "w2": r.standard_normal((64, 64)) * 0.2, "b2": 0.1 * r.standard_normal(64),
            "ln2_g": 1 + 0.1 * r.standard_normal(64), "ln2_b": 0.1 * r.standard_normal(64),
            "w3": r.standard_normal(64) * 0.2, "b3": np.zeros(())}


def torch_critic(w, device):
    """critic_weights' network as a torch fp32 module (the reference's VNet)"""
    nn = torch.nn
    m = nn.Sequential(nn.LayerNorm(29), nn.Linear(29, 64), nn.Tanh(), nn.LayerNorm(64), nn.Linear(64, 64), nn.Tanh(), nn.LayerNorm(64),
                      nn.Linear(64, 1))
    t = lambda k, shape: torch.as_tensor(np.asarray(w[k], dtype=np.float32)).reshape(shape)
    with torch.no_grad():
        for mod, (wk, bk) in zip((m[0], m[1], m[3], m[4], m[6], m[7]), (("ln0_g", "ln0_b"), ("w1", "b1"), ("ln1_g", "ln1_b"), ("w2", "b2"),
                                                                        ("ln2_g", "ln2_b"), ("w3", "b3"))):
            mod.weight.copy_(t(wk, mod.weight.shape))
            mod.bias.copy_(t(bk, mod.bias.shape))
    return m.to(device).train()


def main():
    eng, _, _ = bench.build_engine(N, 672, 0, seed=99, debug_flags=0)
    w = critic_weights()
    eng.set_critic(w, VALUE_NORM)
    dev = eng.device
    net = torch_critic(w, dev)
    mean, scale = VALUE_NORM[0], float(np.sqrt(np.float32(VALUE_NORM[1])))
    out = dict(what="critic_grad", n_envs=N, mfma_per_wavefront_pass=MFMA_PER_PASS)
    g = torch.Generator(device=dev).manual_seed(5)
    from dc_rl_amd.engine import OnPolicyBatch
    for T in (672, 105):
        share = torch.randn((T + 1, N, 29), generator=g, device=dev)
        raw = eng.critic_raw_values(share)
        vp = (raw + 0.3 * torch.randn(raw.shape, generator=g, device=dev)).contiguous()
        ret = (mean + scale * (raw[:T] + 1.2 * torch.randn((T, N), generator=g, device=dev))).contiguous()
        fields = {k: None for k in OnPolicyBatch.FIELDS}
        fields.update(share_obs=share, value_preds=vp, returns=ret, actions=torch.empty((T, N, 3), dtype=torch.int32, device=dev))
        batch = OnPolicyBatch(**fields)
        dense = share[:T].reshape(T * N, 29)
        vp1, ret1 = vp[:T].reshape(-1), ret.reshape(-1)

        def torch_route():
            net.zero_grad(set_to_none=True)
            values = net(dense)[:, 0]
            clipped = vp1 + (values - vp1).clamp(-CLIP, CLIP)
            target = (ret1 - mean) / scale
            ec, eo = target - clipped, target - values
            huber = lambda e: (abs(e) <= DELTA).float() * e ** 2 / 2 + (abs(e) > DELTA).float() * DELTA * (abs(e) - DELTA / 2)
            torch.max(huber(eo), huber(ec)).mean().backward()
            return [p.grad for p in net.parameters()]

        ours = lambda: eng.critic_grads(batch, CLIP, DELTA)
        ours(), torch_route()
        torch.cuda.synchronize()
        # the two routes agree as far as two fp32 summation orders of T N terms do; the figure is reported
        mine_flat = ours()[0].flat
        theirs_flat = torch.cat([p.reshape(-1) for p in torch_route()])
        out[f"max_diff_over_max_grad_{T}"] = float((mine_flat - theirs_flat).abs().max()) / float(theirs_flat.abs().max())
        assert out[f"max_diff_over_max_grad_{T}"] <= 1e-2
        mine, theirs = alternated(ours, torch_route)
        dvalue = eng.value_loss(raw[:T].contiguous(), vp[:T], ret, CLIP, DELTA).dvalue
        one, _ = alternated(lambda: eng.critic_backward(share[:T], dvalue), lambda: None)
        rows = T * N
        out[f"critic_grads_{T}_ms"], out[f"torch_eager_{T}_ms"] = mine, theirs
        out[f"ratio_{T}"] = theirs[0] / mine[0]
        out[f"critic_backward_{T}_ms"] = one
        out[f"critic_backward_{T}_mfma_floor_ms"] = rows / MFMA_FLOOR_ROWS_PER_S * 1e3
        del share, raw, vp, ret, dense, batch
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
