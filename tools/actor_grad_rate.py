"""Measurement: what a HAPPO / MAPPO trainer pays for one agent's actor gradient over the observations it stored.
  * SdcEngine.actor_grads for one agent over [672, 4096] and [105, 4096] rows (evaluate_actions of that agent, ppo_terms, ppo_dlogp,
    actor_backward: the agent's rows read in place, 78 floats apart) against the same network as a torch fp32 eager module doing
    forward, the loss of harl/algorithms/actors/happo.py:56-91 and backward on the same device -- the rows given to torch as a dense
    [T N, 26] buffer, as a HARL actor buffer keeps them;
  * the sdc_actor_backward call on its own (three launches: the gradient kernel, the fp64 sum of the partials, grad_sq), next to the
    gradient kernel's floor from the matrix instructions alone: 300 v_mfma_f32_16x16x4_f32 of 32 cycles per wavefront and 16 rows
    (forward 28 + 64; backward dY1 64, dW2 64, dW3 16, dW1 32, the feature LayerNorm's dX 32), ONE wavefront on each of four SIMDs of
    256 CUs at 2.4 GHz.
ONE process; device events around each call; after one warm-up of every route the median [min, max] of nine, the two routes alternated.
One JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import bench
from actor_eval_rate import N, alternated, torch_actor

AGENT = 1
MFMA_PER_PASS = 28 + 64 + 64 + 64 + 16 + 32 + 32
MFMA_FLOOR_ROWS_PER_S = 256 * 4 * 16 / (MFMA_PER_PASS * 32 / 2.4e9)
CLIP, ENTROPY_COEF = 0.2, 0.01


def main():
    eng, _, _ = bench.build_engine(N, 672, 0, seed=99, debug_flags=0)
    weights = bench.actor_weights()
    for a, w in enumerate(weights):
        eng.set_actor(a, w)
    dev = eng.device
    net = torch_actor(weights[AGENT], dev).train()
    out = dict(what="actor_grad", n_envs=N, agent=AGENT, mfma_per_wavefront_pass=MFMA_PER_PASS)
    g = torch.Generator(device=dev).manual_seed(5)
    from dc_rl_amd.engine import OnPolicyBatch
    for T in (672, 105):
        obs = torch.randn((T + 1, N, 3, 26), generator=g, device=dev)
        acts = torch.randint(0, 3, (T, N, 3), generator=g, device=dev, dtype=torch.int32)
        _, lp, _ = eng.evaluate_actions(obs[:T], acts, agents=(AGENT,))
        old = (lp + 0.1 * torch.randn(lp.shape, generator=g, device=dev)).contiguous()
        adv = torch.randn((T, N), generator=g, device=dev)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        fields = {k: None for k in OnPolicyBatch.FIELDS}
        fields.update(obs=obs, actions=acts, action_log_probs=old, advantages=adv, adv_mean=zero, adv_std=zero + (1.0 - 1e-5))
        batch = OnPolicyBatch(**fields)
        dense = obs[:T, :, AGENT].reshape(T * N, 26).contiguous()
        a64 = acts[:, :, AGENT].reshape(-1, 1).long()
        old1, adv1 = old[:, :, AGENT].reshape(-1, 1), batch.normalized_advantages().reshape(-1, 1)

        def torch_route():
            net.zero_grad(set_to_none=True)
            ls = torch.log_softmax(net(dense), -1)
            imp = torch.exp(ls.gather(-1, a64) - old1)
            loss = -torch.min(imp * adv1, torch.clamp(imp, 1.0 - CLIP, 1.0 + CLIP) * adv1).mean()
            entropy = -(ls.exp() * ls).sum(-1).mean()
            (loss - ENTROPY_COEF * entropy).backward()
            return [p.grad for p in net.parameters()]

        ours = lambda: eng.actor_grads(batch, AGENT, CLIP, ENTROPY_COEF)
        ours(), torch_route()
        torch.cuda.synchronize()
        # the two routes agree as far as two fp32 summation orders of T N cancelling terms do (random rows and advantages: the mean's
        # terms are of order 1 / (T N) each, their sum of order 1 / sqrt(T N)); the figure is reported
        mine_flat = ours()[0].flat
        theirs_flat = torch.cat([p.reshape(-1) for p in torch_route()])
        out[f"max_diff_over_max_grad_{T}"] = float((mine_flat - theirs_flat).abs().max()) / float(theirs_flat.abs().max())
        assert out[f"max_diff_over_max_grad_{T}"] <= 1e-2
        mine, theirs = alternated(ours, torch_route)
        dlogp = eng.ppo_dlogp(AGENT, lp, old, batch.normalized_advantages(), CLIP)
        dent = -ENTROPY_COEF / (T * N)
        one, _ = alternated(lambda: eng.actor_backward(AGENT, obs[:T], acts, dlogp, dent, per_agent=True), lambda: None)
        rows = T * N
        out[f"actor_grads_{T}_ms"], out[f"torch_eager_{T}_ms"] = mine, theirs
        out[f"ratio_{T}"] = theirs[0] / mine[0]
        out[f"actor_backward_{T}_ms"] = one
        out[f"actor_backward_{T}_mfma_floor_ms"] = rows / MFMA_FLOOR_ROWS_PER_S * 1e3
        del obs, acts, dense, batch
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
