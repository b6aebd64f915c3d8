"""Measurement: what a HAPPO / MAPPO trainer pays for the LAST link of an update, the optimiser step, and for a whole update.
  * SdcEngine.actor_adam_step / critic_adam_step on their own (two launches: sum of squares and Adam over the 6391 / 6459
    parameters, then the rewrite of the three / two packed copies);
  * a whole SdcEngine.actor_update and critic_update over [672, 4096] rows and over one eighth of that, [84, 4096] -- a mini-batch of the
    reference's default schedule (8 mini-batches);
  * the path without the device step, on the same inputs: actor_grads, ActorGrads.clip_, assign_to, torch.optim.Adam on a module on the
    device, set_actor with the module's state_dict (the critic likewise) -- what a caller did before the step existed.  Its cost is host
    time, so every figure here is taken twice: between device events and by the wall clock around the call and a synchronisation.
An engine without actor_adam_step (the commit before the step) runs the last route alone: that is how the two commits are compared.
ONE process; after one warm-up of every route the median [min, max] of nine, the routes alternated.  One JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bench
from actor_eval_rate import N, torch_actor
from critic_grad_rate import CLIP, DELTA, VALUE_NORM, critic_weights, torch_critic

AGENT, ENTROPY_COEF, LR, EPS, MAX_NORM, REPS = 1, 0.01, 5e-4, 1e-5, 10.0, 9


def timed(routes, reps=REPS):
    """{name: fn} -> {name: {"event_ms": [median, min, max], "wall_ms": [...]}}, the routes in turn, each between device events and
    under the wall clock up to a synchronisation behind it"""
    ts = {k: ([], []) for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k][1].append((time.perf_counter() - t0) * 1e3)
            ts[k][0].append(e0.elapsed_time(e1))
    three = lambda x: [float(np.median(x)), float(min(x)), float(max(x))]
    return {k: dict(event_ms=three(ev), wall_ms=three(wall)) for k, (ev, wall) in ts.items()}


def named(net, keys):
    """a Sequential of actor_eval_rate / critic_grad_rate under the reference's state_dict keys"""
    return dict(zip(keys, (p for mod in net if list(mod.parameters()) for p in (mod.weight, mod.bias))))


def main():
    from dc_rl_amd.engine import _ACTOR_SD_KEYS, _CRITIC_SD_KEYS, OnPolicyBatch
    eng, _, _ = bench.build_engine(N, 672, 0, seed=99, debug_flags=0)
    weights, cw = bench.actor_weights(), critic_weights()
    for a, w in enumerate(weights):
        eng.set_actor(a, w)
    eng.set_critic(cw, VALUE_NORM)
    dev = eng.device
    device_step = hasattr(eng, "actor_adam_step")
    out = dict(what="update", n_envs=N, agent=AGENT, device_step=device_step)
    g = torch.Generator(device=dev).manual_seed(5)
    # the host path's modules: parameters under the reference's keys, in the structs' order
    anet, cnet = torch_actor(weights[AGENT], dev).train(), torch_critic(cw, dev)
    akeys = [_ACTOR_SD_KEYS[k] for k in ("ln0_gamma", "ln0_beta", "w1", "b1", "ln1_gamma", "ln1_beta", "w2", "b2", "ln2_gamma", "ln2_beta", "w3", "b3")]
    ckeys = [_CRITIC_SD_KEYS[k] for k in ("ln0_g", "ln0_b", "w1", "b1", "ln1_g", "ln1_b", "w2", "b2", "ln2_g", "ln2_b", "w3", "b3")]
    aparams, cparams = named(anet, akeys), named(cnet, ckeys)
    aopt = torch.optim.Adam(aparams.values(), lr=LR, eps=EPS)
    copt = torch.optim.Adam(cparams.values(), lr=LR, eps=EPS)

    class Module:      # (what assign_to asks of a module: named_parameters under the reference's keys)
        def __init__(self, params):
            self.params = params

        def named_parameters(self):
            return self.params.items()

    amod, cmod = Module(aparams), Module(cparams)
    for T in (672, 84):
        obs = torch.randn((T + 1, N, 3, 26), generator=g, device=dev)
        acts = torch.randint(0, 3, (T, N, 3), generator=g, device=dev, dtype=torch.int32)
        _, lp, _ = eng.evaluate_actions(obs[:T], acts, agents=(AGENT,))
        old = (lp + 0.1 * torch.randn(lp.shape, generator=g, device=dev)).contiguous()
        share = torch.randn((T + 1, N, 29), generator=g, device=dev)
        raw = eng.critic_raw_values(share)
        vp = (raw + 0.3 * torch.randn(raw.shape, generator=g, device=dev)).contiguous()
        ret = (VALUE_NORM[0] + 7.5 * (raw[:T] + 1.2 * torch.randn((T, N), generator=g, device=dev))).contiguous()
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        fields = {k: None for k in OnPolicyBatch.FIELDS}
        fields.update(obs=obs, actions=acts, action_log_probs=old, advantages=torch.randn((T, N), generator=g, device=dev), adv_mean=zero,
                      adv_std=zero + (1.0 - 1e-5), share_obs=share, value_preds=vp, returns=ret)
        batch = OnPolicyBatch(**fields)

        def host_actor():
            grads, _ = eng.actor_grads(batch, AGENT, CLIP, ENTROPY_COEF)
            grads.clip_(MAX_NORM)
            grads.assign_to(amod)
            aopt.step()
            eng.set_actor(AGENT, dict({k: p.detach() for k, p in aparams.items()}, activation="tanh"))

        def host_critic():
            grads, _ = eng.critic_grads(batch, CLIP, DELTA)
            grads.clip_(MAX_NORM)
            grads.assign_to(cmod)
            copt.step()
            eng.set_critic({k: p.detach() for k, p in cparams.items()}, VALUE_NORM)

        routes = {"host_actor_update": host_actor, "host_critic_update": host_critic,
                  "actor_grads": lambda: eng.actor_grads(batch, AGENT, CLIP, ENTROPY_COEF), "critic_grads": lambda: eng.critic_grads(batch, CLIP, DELTA)}
        if device_step:
            kw = dict(lr=LR, eps=EPS, max_grad_norm=MAX_NORM)
            ga, gc = eng.actor_grads(batch, AGENT, CLIP, ENTROPY_COEF)[0], eng.critic_grads(batch, CLIP, DELTA)[0]
            routes.update({"actor_update": lambda: eng.actor_update(batch, AGENT, CLIP, ENTROPY_COEF, **kw),
                           "critic_update": lambda: eng.critic_update(batch, CLIP, DELTA, **kw),
                           "actor_adam_step": lambda: eng.actor_adam_step(AGENT, ga, **kw),
                           "critic_adam_step": lambda: eng.critic_adam_step(gc, **kw)})
        for fn in routes.values():      # (one warm-up of every route)
            fn()
        torch.cuda.synchronize()
        out["rows_%d" % T] = timed(routes)
        del obs, acts, share, batch
    if device_step:
        st = eng.optim_state(AGENT)
        out["actor_steps_taken"], out["actor_steps_skipped"] = st["step"], st["skipped"]
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
