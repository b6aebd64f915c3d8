"""Measurement: what a HAPPO / MAPPO trainer pays to run the actors again over the observations it stored, and to build the PPO terms.
  * SdcEngine.evaluate_actions over [672, 4096] and [105, 4096] rows of three agents (three sdc_actor_evaluate launches reading the
    agents' rows in place, 78 floats apart, and one sdc_action_log_probs) against the same three networks as torch fp32 eager modules
    on the same rows -- given to torch as dense [T N, 26] buffers per agent, as a HARL actor buffer keeps them -- followed by
    log_softmax, the gather of the played action and the entropy;
  * SdcEngine.ppo_terms over [672, 4096] (both launches) against the torch ops of harl/algorithms/actors/happo.py:66-86 and the
    runner's factor update, on the same arrays;
  * one sdc_actor_evaluate launch on its own: achieved matrix TFLOP/s (2 (26 64 + 64 64 + 64 3) per row) and TB/s (a row's 104 bytes
    in, 12 out), next to the launch's floor from the matrix instructions alone (92 v_mfma_f32_16x16x4_f32 of 32 cycles per wavefront
    and 16 rows, four SIMDs on each of 256 CUs at 2.4 GHz).
ONE process; device events around each call; after one warm-up of every route the median [min, max] of nine, the two routes alternated.
One JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench

REPS = 9
N = 4096
FLOP_PER_ROW = 2 * (26 * 64 + 64 * 64 + 64 * 3)
BYTES_PER_ROW = 26 * 4 + 3 * 4
MFMA_FLOOR_ROWS_PER_S = 256 * 4 * 16 / (92 * 32 / 2.4e9)


def torch_actor(w, device):
    """bench.actor_weights' network as a torch fp32 module (the reference's StochasticPolicy up to the logits)"""
    nn = torch.nn
    m = nn.Sequential(nn.LayerNorm(26), nn.Linear(26, 64), nn.Tanh(), nn.LayerNorm(64), nn.Linear(64, 64), nn.Tanh(), nn.LayerNorm(64),
                      nn.Linear(64, 3))
    t = lambda k: torch.as_tensor(np.asarray(w[k], dtype=np.float32))
    with torch.no_grad():
        for mod, (wk, bk) in zip((m[0], m[1], m[3], m[4], m[6], m[7]), (("ln0_gamma", "ln0_beta"), ("w1", "b1"), ("ln1_gamma", "ln1_beta"),
                                                                        ("w2", "b2"), ("ln2_gamma", "ln2_beta"), ("w3", "b3"))):
            mod.weight.copy_(t(wk))
            mod.bias.copy_(t(bk))
    return m.to(device).eval()


def alternated(a, b, reps=REPS):
    """(median, min, max) ms of a() and of b() between device events, a and b in turn"""
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((a, ta), (b, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    three = lambda ts: [float(np.median(ts)), float(min(ts)), float(max(ts))]
    return three(ta), three(tb)


def main():
    eng, _, _ = bench.build_engine(N, 672, 0, seed=99, debug_flags=0)
    weights = bench.actor_weights()
    for a, w in enumerate(weights):
        eng.set_actor(a, w)
    dev = eng.device
    nets = [torch_actor(w, dev) for w in weights]
    out = dict(what="actor_eval", n_envs=N)
    g = torch.Generator(device=dev).manual_seed(5)
    for T in (672, 105):
        obs = torch.randn((T, N, 3, 26), generator=g, device=dev)
        acts = torch.randint(0, 3, (T, N, 3), generator=g, device=dev, dtype=torch.int32)
        dense = [obs[:, :, a].reshape(T * N, 26).contiguous() for a in range(3)]
        acts64 = acts.long()

        def torch_route():
            with torch.no_grad():
                lp, ent = [], []
                for a in range(3):
                    ls = torch.log_softmax(nets[a](dense[a]), -1)
                    lp.append(ls.gather(-1, acts64[:, :, a].reshape(-1, 1)))
                    ent.append(-(ls.exp() * ls).sum(-1))
                return lp, ent

        ours = lambda: eng.evaluate_actions(obs, acts)
        ours(), torch_route()
        torch.cuda.synchronize()
        # the two routes agree (fp32, another summation order)
        lg, lp, _ = ours()
        assert float((lp[:, :, 1].reshape(-1, 1) - torch_route()[0][1]).abs().max()) < 1e-3
        mine, theirs = alternated(ours, torch_route)
        one, _ = alternated(lambda: eng.actor_logits(1, obs), lambda: None)
        rows = T * N
        out[f"evaluate_actions_{T}_ms"], out[f"torch_eager_{T}_ms"] = mine, theirs
        out[f"ratio_{T}"] = theirs[0] / mine[0]
        out[f"one_launch_{T}_ms"] = one
        out[f"one_launch_{T}_TFLOPs"] = rows * FLOP_PER_ROW / one[0] / 1e9
        out[f"one_launch_{T}_TBps"] = rows * BYTES_PER_ROW / one[0] / 1e9
        out[f"one_launch_{T}_mfma_floor_ms"] = rows / MFMA_FLOOR_ROWS_PER_S * 1e3
        if T == 672:
            old = (lp + 0.1 * torch.randn(lp.shape, generator=g, device=dev)).contiguous()
            adv = torch.randn((T, N), generator=g, device=dev)
            factor = torch.exp(0.1 * torch.randn((T, N), generator=g, device=dev))
            ent = eng.action_log_probs(acts, lg)[1]

            def torch_terms():
                new1, old1, e1 = lp[:, :, 1].reshape(-1, 1), old[:, :, 1].reshape(-1, 1), ent[:, :, 1]
                f, A = factor.reshape(-1, 1), adv.reshape(-1, 1)
                imp = torch.prod(torch.exp(new1 - old1), dim=-1, keepdim=True)
                surr1 = imp * A
                surr2 = torch.clamp(imp, 1.0 - 0.2, 1.0 + 0.2) * A
                loss = -torch.sum(f * torch.min(surr1, surr2), dim=-1, keepdim=True).mean()
                return loss, e1.mean(), f * imp

            terms = lambda: eng.ppo_terms(1, lp, old, adv, 0.2, factor=factor, entropy=ent)
            terms(), torch_terms()
            torch.cuda.synchronize()
            assert abs(terms().summary()["policy_loss"] - float(torch_terms()[0])) < 1e-4
            mine, theirs = alternated(terms, torch_terms)
            out["ppo_terms_672_ms"], out["torch_ops_672_ms"] = mine, theirs
            out["ppo_terms_ratio"] = theirs[0] / mine[0]
            out["ppo_terms_TBps"] = rows * (4 * 4 + 3 * 4 + 4) / mine[0] / 1e9      # (5 dwords in -- one per 12-byte stride --, 3 out)
        del obs, acts, dense
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
