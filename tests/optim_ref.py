"""sdc_actor_adam_step / sdc_critic_adam_step restated in NumPy (include/sustaindc_hip.h THE OPTIMISER STEP; TEST INFRASTRUCTURE, never
imported by the product): the fixed-order fp64 sum of squares, the scalar preparation with Python floats (fp64), and the step per element
in np.float32, ONE operation per line so that nothing contracts and every result is rounded once.  tests/test_optim_ref.py holds it to
torch.optim.Adam, tests/test_optim_abi.py holds csrc/sdc_optim.hpp to it bit for bit on the host, tests/test_gpu_optim.py the kernel.
A plain module: no GPU; torch is imported by `torch_run` alone."""
import functools
import math
import os

import numpy as np

SQ_LANES = 256          # csrc/sdc_optim.hpp SDC_ADAM_SQ_LANES
F = np.float32


def new_state():
    """sdc_optim_state from new"""
    return dict(step=0, beta1_pow=1.0, beta2_pow=1.0, skipped=0)


def grad_sq(g):
    """the header's order over any length: lane l adds (double)g[j] * (double)g[j] for j = l, l + 256, ...; then half = 128 .. 1"""
    g = np.asarray(g)
    assert g.dtype == np.float32 and g.ndim == 1
    v = g.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = v * v
        K = (g.size + SQ_LANES - 1) // SQ_LANES
        pad = np.zeros(K * SQ_LANES)
        pad[:g.size] = sq
        pad = pad.reshape(K, SQ_LANES)
        acc = np.zeros(SQ_LANES)
        for k in range(K):
            acc = acc + pad[k]      # (a lane past the end keeps its sum: + 0.0 leaves a non-negative sum, a NaN and an infinity as they are)
        half = SQ_LANES // 2
        while half >= 1:
            acc[:half] = acc[:half] + acc[half:2 * half]
            half //= 2
    return float(acc[0])


def prepare(S, state, lr, beta1, beta2, eps, weight_decay, max_grad_norm):
    """steps 2 to 4: None (and skipped += 1) for an S that is not finite, else the fp32 scalars; `state` moves on in place"""
    if not math.isfinite(S):
        state["skipped"] += 1
        return None
    norm = math.sqrt(S)
    ratio = float(max_grad_norm) / (norm + 1e-6)
    c = ratio if ratio < 1.0 else 1.0
    state["step"] += 1
    state["beta1_pow"] = state["beta1_pow"] * float(beta1)
    state["beta2_pow"] = state["beta2_pow"] * float(beta2)
    return dict(clip=F(c), weight_decay=F(weight_decay), one_minus_beta1=F(1.0 - float(beta1)), beta2=F(beta2),
                one_minus_beta2=F(1.0 - float(beta2)), rsq=F(math.sqrt(1.0 - state["beta2_pow"])), eps=F(eps),
                step_size=F(float(lr) / (1.0 - state["beta1_pow"])))


def elements(k, g, p, m, v):
    """step 5 over fp32 arrays -> (p, m, v), new arrays"""
    assert all(a.dtype == np.float32 for a in (g, p, m, v))
    with np.errstate(all="ignore"):
        g = g * k["clip"]
        if k["weight_decay"] != F(0.0):
            wp = k["weight_decay"] * p
            g = g + wp
        dm = g - m
        wdm = k["one_minus_beta1"] * dm
        m = m + wdm
        v = v * k["beta2"]
        bg = k["one_minus_beta2"] * g
        bgg = bg * g
        v = v + bgg
        root = np.sqrt(v)
        scaled = root / k["rsq"]
        denom = scaled + k["eps"]
        q = m / denom
        upd = k["step_size"] * q
        p = p - upd
    assert all(a.dtype == np.float32 for a in (p, m, v))
    return p, m, v


def step(g, p, m, v, state, lr, betas=(0.9, 0.999), eps=1e-5, weight_decay=0.0, max_grad_norm=None, first=0):
    """one step of the contract: fp32 arrays in, (p, m, v, sqrt(S)) out (new arrays); `state` (a dict as new_state's) moves on in
    place; the `first` leading elements are left alone (a network whose feature LayerNorm is off: its ln0 entries)"""
    g, p, m, v = (np.ascontiguousarray(a, dtype=np.float32) for a in (g, p, m, v))
    S = grad_sq(g)
    with np.errstate(invalid="ignore"):
        norm = float(np.sqrt(np.float64(S)))
    k = prepare(S, state, lr, betas[0], betas[1], eps, weight_decay, math.inf if max_grad_norm is None else max_grad_norm)
    if k is None:
        return p.copy(), m.copy(), v.copy(), norm
    p2, m2, v2 = p.copy(), m.copy(), v.copy()
    p2[first:], m2[first:], v2[first:] = elements(k, g[first:], p[first:], m[first:], v[first:])
    return p2, m2, v2, norm


def torch_run(grads, p0, dtype, lr, betas, eps, weight_decay, max_grad_norm):
    """torch.optim.Adam(foreach=False, fused=False) behind clip_grad_norm_ on the CPU over the list of gradients -> the parameters
    after every step, as fp64 arrays"""
    import torch
    p = torch.nn.Parameter(torch.tensor(np.asarray(p0), dtype=dtype))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False, fused=False)
    out = []
    for g in grads:
        p.grad = torch.tensor(np.asarray(g), dtype=dtype)
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_([p], max_grad_norm, foreach=False)
        opt.step()
        out.append(p.detach().to(torch.float64).numpy().copy())
    return out


# ---- the fixture the reference wrote (tests/golden/optim/optim.npz, tests/golden/gen_optim_golden.py) --------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim", "optim.npz")
UPDATES = 3


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def fixture_hyper():
    """the reference's optimiser arguments as `step` takes them"""
    fx = fixture()
    return dict(lr=float(fx["lr"]), betas=(0.9, 0.999), eps=float(fx["opti_eps"]), weight_decay=float(fx["weight_decay"]),
                max_grad_norm=float(fx["max_grad_norm"]))


def actor_case():
    """the actor's inputs (tests/golden/actor_grad/actor_grad.npz, the configuration the fixture names) -> (activation, feature_norm, case)"""
    from tests import actor_grad_ref as AG
    act, fn = str(fixture()["actor_config"]).split("_fn")
    return act, bool(int(fn)), AG.case(act, bool(int(fn)))


def critic_case():
    """the critic's inputs (tests/golden/critic_grad/critic_grad.npz) -> (activation, feature_norm, case)"""
    from tests import critic_grad_ref as CG
    cfg, loss = str(fixture()["critic_config"]).split("_", 2)[:2], str(fixture()["critic_config"]).split("_", 2)[2]
    act, fn = cfg[0], bool(int(cfg[1][2:]))
    return act, fn, CG.case(act, fn, loss)


def sd_flat(sd, fields, keys, shapes):
    """a state_dict -> fp32 [n] in the params struct's order (zeros for an absent feature LayerNorm)"""
    return np.concatenate([np.asarray(sd[keys[k]], dtype=np.float32).reshape(-1) if keys[k] in sd else np.zeros(int(np.prod(shapes[k])), np.float32)
                           for k in fields])


def flat_sd(flat, like, fields, keys, shapes):
    """fp32 [n] -> a state_dict of arrays with the keys and shapes of `like`"""
    out, at = {}, 0
    for k in fields:
        n = int(np.prod(shapes[k]))
        if keys[k] in like:
            out[keys[k]] = flat[at:at + n].reshape(np.asarray(like[keys[k]]).shape).copy()
        at += n
    return out


def fixture_distance(results, which):
    """the largest |p - p64| over the fixture's updates for `results` [UPDATES] of flat fp32 parameters in the struct's order, and the
    same for the reference's own fp32 results -> (distance, the reference's)"""
    fx = fixture()
    first = {"actor": 6391, "critic": 6459}[which] - fx["%s_p64_1" % which].size      # (the fixture holds no ln0 entries for a network without)
    d = max(float(np.abs(np.asarray(r, np.float64)[first:] - fx["%s_p64_%d" % (which, u + 1)]).max()) for u, r in enumerate(results))
    d32 = max(float(np.abs(fx["%s_p32_%d" % (which, u)].astype(np.float64) - fx["%s_p64_%d" % (which, u)]).max()) for u in range(1, UPDATES + 1))
    return d, d32
