"""sdc_actor_backward and sdc_ppo_dlogp restated in NumPy fp64 (include/sustaindc_hip.h THE ACTORS' GRADIENT; TEST INFRASTRUCTURE, never
imported by the product): the hand-derived backward of the actor network over rows, the `dlogp` rule, and the fixed summation order of
grad_sq; and the fixture the reference wrote (tests/golden/actor_grad/actor_grad.npz, tests/golden/gen_actor_grad_golden.py).
tests/test_actor_grad_ref.py holds `backward` to torch fp64 autograd and to the reference's own gradients, tests/test_gpu_actor_grad.py
holds the kernels to these functions; both measure against torch autograd through `torch_net` and `torch_grads` below.  A plain module: no
GPU; torch is imported by those two functions alone."""
import functools
import os

import numpy as np

from tests.actor_eval_ref import CONFIGS, EPS, KEYS, R, cfg_name      # noqa: F401  (the configurations and the key names are shared)

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "actor_grad", "actor_grad.npz")
FIELDS = ("ln0_gamma", "ln0_beta", "w1", "b1", "ln1_gamma", "ln1_beta", "w2", "b2", "ln2_gamma", "ln2_beta", "w3", "b3")      # sdc_actor_params' order
SHAPES = {"ln0_gamma": (26,), "ln0_beta": (26,), "w1": (64, 26), "b1": (64,), "ln1_gamma": (64,), "ln1_beta": (64,),
          "w2": (64, 64), "b2": (64,), "ln2_gamma": (64,), "ln2_beta": (64,), "w3": (3, 64), "b3": (3,)}
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES.values())      # 6391: include/sustaindc_hip.h SDC_ACTOR_N_PARAMS
MAX_BLOCKS = 256                                              # include/sustaindc_hip.h SDC_ACTOR_GRAD_MAX_BLOCKS
SQ_BLOCK = 256                                                # lanes of sdc_actor_grad_sq_kernel


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def case(activation, feature_norm):
    """one configuration's arrays without their prefix, its state_dict under "sd", the reference's gradients under "grad" """
    c = cfg_name(activation, feature_norm) + "_"
    out = {k[len(c):]: v for k, v in fixture().items() if k.startswith(c)}
    out["sd"] = {k[len("sd_"):]: v for k, v in out.items() if k.startswith("sd_")}
    out["grad"] = {k[len("grad_"):]: v for k, v in out.items() if k.startswith("grad_")}
    return out


def dlogp_rule(r, A, F, scale, clip_param):
    """the header's rule from the ratio on, fp64 arrays, one NumPy operation per operation -> (d fp64, open bool)"""
    lo, hi = 1.0 - float(clip_param), 1.0 + float(clip_param)      # (1 -+ clip in double, as the library forms them)
    s1 = r * A
    rc = np.where(r < lo, lo, r)
    rc = np.where(rc > hi, hi, rc)
    s2 = rc * A
    clipped = (r < lo) | (r > hi)
    is_open = ~clipped | (s1 < s2)
    d = -(((scale * F) * A) * r)
    return np.where(is_open, d, 0.0), is_open


def dlogp(new_log_probs, old_log_probs, advantages, agent, clip_param, factor=None, scale=None, fp32_inputs=True):
    """new / old [..., 3] fp32 (column `agent`), advantages and factor [...] fp32 -> (dlogp fp32 [...], r fp64, open bool, dlogp fp64).
    `fp32_inputs` False: new_log_probs may be an fp64 restatement's"""
    new, old, adv = np.asarray(new_log_probs), np.asarray(old_log_probs), np.asarray(advantages)
    assert old.dtype == adv.dtype == np.float32 and (new.dtype == np.float32 or not fp32_inputs)
    lr = new[..., agent].astype(np.float64) - old[..., agent].astype(np.float64)
    r = np.exp(lr)
    A = adv.astype(np.float64)
    F = np.ones(adv.shape) if factor is None else np.asarray(factor, dtype=np.float32).astype(np.float64)
    scale = 1.0 / adv.size if scale is None else float(scale)
    d, is_open = dlogp_rule(r, A, F, scale, clip_param)
    return d.astype(np.float32), r, is_open, d


def backward(sd, x, actions, dlogp_rows, dent, activation):
    """The gradient of L = sum_r dlogp[r] logp_r(a_r) + dent sum_r H_r in NumPy fp64, from a state_dict (torch's layout; without a
    feature_norm the ln0 gradients are zeros): x [R, 26], actions [R] (outside 0 .. 2: an all-zero one-hot), dlogp [R] -> a dict of
    the FIELDS' gradients, and under "z1", "z2" the pre-activations, under "logits" the forward's logits"""
    p = {k: np.asarray(sd[v], dtype=np.float64) for k, v in KEYS.items() if v in sd}
    tanh = activation == "tanh"
    act = np.tanh if tanh else (lambda v: np.maximum(v, 0.0))
    dact = (lambda z, a: 1.0 - a * a) if tanh else (lambda z, a: (z > 0.0).astype(np.float64))

    def ln(h):
        mean = h.mean(-1, keepdims=True)
        var = ((h - mean) ** 2).mean(-1, keepdims=True)
        rs = 1.0 / np.sqrt(var + EPS)
        return (h - mean) * rs, rs

    def ln_back(dy, n, rs, gain):
        dn = dy * gain
        dx = rs * (dn - dn.mean(-1, keepdims=True) - n * (dn * n).mean(-1, keepdims=True))
        return (dy * n).sum(0), dy.sum(0), dx

    x = np.asarray(x, dtype=np.float64)
    a_r = np.asarray(actions).reshape(-1).astype(np.int64)
    c_r = np.asarray(dlogp_rows, dtype=np.float64).reshape(-1)
    fn = "ln0_gamma" in p
    if fn:
        n0, rs0 = ln(x)
        xh = n0 * p["ln0_gamma"] + p["ln0_beta"]
    else:
        xh = x
    z1 = xh @ p["w1"].T + p["b1"]
    a1 = act(z1)
    n1, rs1 = ln(a1)
    y1 = n1 * p["ln1_gamma"] + p["ln1_beta"]
    z2 = y1 @ p["w2"].T + p["b2"]
    a2 = act(z2)
    n2, rs2 = ln(a2)
    y2 = n2 * p["ln2_gamma"] + p["ln2_beta"]
    lg = y2 @ p["w3"].T + p["b3"]
    zc = lg - lg.max(-1, keepdims=True)
    logp = zc - np.log(np.exp(zc).sum(-1, keepdims=True))
    pr = np.exp(logp)
    H = -(pr * logp).sum(-1, keepdims=True)
    hot = (a_r[:, None] == np.arange(3)[None, :]).astype(np.float64)
    dl = c_r[:, None] * (hot - pr) - float(dent) * (pr * (logp + H))
    g = {"b3": dl.sum(0), "w3": dl.T @ y2}
    g["ln2_gamma"], g["ln2_beta"], da2 = ln_back(dl @ p["w3"], n2, rs2, p["ln2_gamma"])
    dz2 = da2 * dact(z2, a2)
    g["b2"], g["w2"] = dz2.sum(0), dz2.T @ y1
    g["ln1_gamma"], g["ln1_beta"], da1 = ln_back(dz2 @ p["w2"], n1, rs1, p["ln1_gamma"])
    dz1 = da1 * dact(z1, a1)
    g["b1"], g["w1"] = dz1.sum(0), dz1.T @ xh
    if fn:
        dxh = dz1 @ p["w1"]
        g["ln0_gamma"], g["ln0_beta"] = (dxh * n0).sum(0), dxh.sum(0)
    else:
        g["ln0_gamma"], g["ln0_beta"] = np.zeros(26), np.zeros(26)
    g.update(z1=z1, z2=z2, logits=lg)
    return g


def flat(g, dtype=np.float64):
    """a dict of the FIELDS' gradients -> [6391] in sdc_actor_params' order"""
    return np.concatenate([np.asarray(g[k], dtype=dtype).reshape(-1) for k in FIELDS])


def split(flat_grads):
    """[6391] -> {field: shaped view}"""
    out, at = {}, 0
    for k in FIELDS:
        n = int(np.prod(SHAPES[k]))
        out[k] = np.asarray(flat_grads)[at:at + n].reshape(SHAPES[k])
        at += n
    assert at == N_PARAMS
    return out


def distance(got, want):
    """the measure of the tests: per parameter tensor max|got - want| / max|want| (0 where both are all zero) -> {field: value}"""
    out = {}
    for k in FIELDS:
        a, b = np.asarray(got[k], dtype=np.float64).reshape(-1), np.asarray(want[k], dtype=np.float64).reshape(-1)
        top = np.abs(b).max()
        out[k] = 0.0 if top == 0.0 and not a.any() else float(np.abs(a - b).max() / top)
    return out


def grad_sq(flat32):
    """the header's order: lane l adds (double)g[j] * (double)g[j] for j = l, l + 256, ...; then half = 128 .. 1: lane l takes l + half"""
    g = np.asarray(flat32)
    assert g.dtype == np.float32 and g.shape == (N_PARAMS,)
    v = g.astype(np.float64)
    sq = v * v
    K = (N_PARAMS + SQ_BLOCK - 1) // SQ_BLOCK
    pad = np.zeros(K * SQ_BLOCK)
    pad[:N_PARAMS] = sq
    pad = pad.reshape(K, SQ_BLOCK)
    acc = np.zeros(SQ_BLOCK)
    for k in range(K):
        acc = acc + pad[k]        # (a lane past the end keeps its sum: + 0.0 leaves a non-negative sum as it is)
    half = SQ_BLOCK // 2
    while half >= 1:
        acc[:half] = acc[:half] + acc[half:2 * half]
        half //= 2
    return float(acc[0])


def relu_margin(g):
    """the smallest |pre-activation| of a restated backward: a relu unit whose pre-activation straddles zero flips between fp32 and fp64"""
    return float(min(np.abs(g["z1"]).min(), np.abs(g["z2"]).min()))


def blocks(n_rows):
    """the workgroups (partials) of sdc_actor_backward for n_rows rows"""
    return min((n_rows + 63) // 64, MAX_BLOCKS)


# ---- torch autograd over a plain-torch network of the same shape (the reference arithmetic the tests measure against) -------------------
def torch_net(sd, activation, dtype=None):
    """tests/actor_ref.torch_actor (a plain torch module with the reference's parameter names) holding the state_dict `sd`"""
    import torch
    from tests import actor_ref as AR
    m = AR.torch_actor(1, activation, feature_norm=KEYS["ln0_gamma"] in sd)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    return m.to(dtype) if dtype is not None else m


def torch_grads(net, x, actions, dlogp_rows, dent):
    """d(sum_r dlogp[r] logp_r(a_r) + dent sum_r H_r) / d(parameters) by torch autograd on the CPU in the module's dtype
    -> {field: fp64 array} (ln0 zeros for a module without a feature_norm); an action outside 0 .. 2 is an all-zero one-hot"""
    import torch
    dt = next(net.parameters()).dtype
    net.zero_grad()
    lg = net(torch.as_tensor(np.asarray(x), dtype=dt))
    logp = torch.log_softmax(lg, -1)
    H = -(logp.exp() * logp).sum(-1)
    a = torch.as_tensor(np.asarray(actions).reshape(-1)).long()
    valid = (a >= 0) & (a <= 2)
    # (an all-zero one-hot: sum_c hot_c logit_c - logsumexp = -logsumexp, whose derivative is -p)
    chosen = torch.where(valid, logp.gather(-1, a.clamp(0, 2)[:, None])[:, 0], -torch.logsumexp(lg, -1))
    loss = (torch.as_tensor(np.asarray(dlogp_rows).reshape(-1), dtype=dt) * chosen).sum() + float(dent) * H.sum()
    loss.backward()
    inv = {v: k for k, v in KEYS.items()}
    g = {inv[n]: p.grad.detach().numpy().astype(np.float64) for n, p in net.named_parameters()}
    for k in ("ln0_gamma", "ln0_beta"):
        g.setdefault(k, np.zeros(26))
    return g
