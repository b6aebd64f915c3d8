"""sdc_value_loss and sdc_critic_backward restated in NumPy fp64 (include/sustaindc_hip.h THE CRITIC'S GRADIENT; TEST INFRASTRUCTURE, never
imported by the product): the value-loss rule element by element, the hand-derived backward of the critic over tests/critic_ref.py's
forward, the fixed summation order of grad_sq and of the eight statistics; and the fixture the reference wrote
(tests/golden/critic_grad/critic_grad.npz, tests/golden/gen_critic_grad_golden.py).  tests/test_critic_grad_ref.py holds these to torch
fp64 autograd and to the reference's own gradients, tests/test_gpu_critic_grad.py holds the kernels to these functions; both measure
against torch autograd through `torch_net`, `torch_value_loss` and `torch_grads` below.  A plain module: no GPU; torch is imported by those
functions alone."""
import functools
import os

import numpy as np

from tests.critic_ref import EPS, H, IN, KEYS

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "critic_grad", "critic_grad.npz")
R = 67
CONFIGS = [("tanh", True), ("tanh", False), ("relu", True), ("relu", False)]
FIELDS = ("ln0_g", "ln0_b", "w1", "b1", "ln1_g", "ln1_b", "w2", "b2", "ln2_g", "ln2_b", "w3", "b3")      # sdc_critic_params' order
SHAPES = {"ln0_g": (29,), "ln0_b": (29,), "w1": (64, 29), "b1": (64,), "ln1_g": (64,), "ln1_b": (64,),
          "w2": (64, 64), "b2": (64,), "ln2_g": (64,), "ln2_b": (64,), "w3": (64,), "b3": ()}
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES.values())      # 6459: include/sustaindc_hip.h SDC_CRITIC_N_PARAMS
MAX_BLOCKS = 256                                              # include/sustaindc_hip.h SDC_CRITIC_GRAD_MAX_BLOCKS
SQ_BLOCK = 256                                                # lanes of sdc_critic_grad_sq_kernel
HUBER, CLIPPED = 1, 2                                         # sdc_value_loss' flags


def cfg_name(activation, feature_norm):
    return "%s_fn%d" % (activation, int(feature_norm))


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def case(activation, feature_norm, loss="huber_clip"):
    """one configuration's arrays without their prefix (`loss`: "huber_clip" or "mse"), its state_dict under "sd", the reference's
    gradients under "grad" """
    c = "%s_%s_" % (cfg_name(activation, feature_norm), loss)
    out = {k[len(c):]: v for k, v in fixture().items() if k.startswith(c)}
    out["sd"] = {k[len("sd_"):]: v for k, v in out.items() if k.startswith("sd_")}
    out["grad"] = {k[len("grad_"):]: v for k, v in out.items() if k.startswith("grad_")}
    return out


# ---- the value loss ---------------------------------------------------------------------------------------------------------------------
def value_loss(raw, value_preds, returns, scale, shift, clip, delta, flags, coef):
    """the header's rule, one NumPy fp64 operation per operation, from fp32 arrays (fp64 inputs are taken as they are: an fp64
    restatement's raw values) -> a dict: loss, dvalue (fp32, each rounded once), L, g, t, eo, ec, lo, lc, d (fp64)"""
    u, vp, ret = (np.asarray(a).astype(np.float64) for a in (raw, value_preds, returns))
    clip, delta, coef, scale, shift = float(clip), float(delta), float(coef), float(scale), float(shift)
    huber = bool(flags & HUBER)

    def l(e):
        sq = (e * e) / 2.0
        if not huber:
            return sq
        a = np.where(e < 0.0, -e, e)
        return np.where(a <= delta, sq, delta * (a - delta / 2.0))

    def dl(e):
        if not huber:
            return e
        a = np.where(e < 0.0, -e, e)
        return np.where(a <= delta, e, np.where(e > 0.0, delta, -delta))

    t = (ret - shift) / scale
    d = u - vp
    dc = np.where(d < -clip, -clip, np.where(d > clip, clip, d))
    uc = vp + dc
    eo, ec = t - u, t - uc
    lo, lc = l(eo), l(ec)
    go = -dl(eo)
    gc = np.where((-clip <= d) & (d <= clip), -dl(ec), 0.0)
    if flags & CLIPPED:
        L = np.where(lo > lc, lo, lc)
        g = np.where(lo > lc, go, np.where(lo < lc, gc, 0.5 * go + 0.5 * gc))
    else:
        L, g = lo, go
    return dict(loss=L.astype(np.float32), dvalue=(coef * g).astype(np.float32), L=L, g=g, t=t, eo=eo, ec=ec, lo=lo, lc=lc, d=d, u=u)


def stats(v):
    """the eight statistics of a `value_loss` result in the kernels' fixed two-stage order (tests/ppo_ref.ordered): from the STORED fp32
    loss and the fp64 terms"""
    from tests.ppo_ref import ordered
    eo = v["eo"]
    return np.array([ordered(v["loss"].astype(np.float64), "sum"), ordered(v["u"], "sum"), ordered(eo, "sum"), ordered(eo * eo, "sum"),
                     ordered((v["lc"] > v["lo"]).astype(np.float64), "sum"), ordered(eo, "min"), ordered(eo, "max"), float(eo.size)])


def summary(s):
    """ValueLossTerms.summary from stats [8]"""
    n = float(s[7])
    return dict(value_loss=float(s[0]) / n, value_mean=float(s[1]) / n, error_mean=float(s[2]) / n, error_rms=float(np.sqrt(float(s[3]) / n)),
                clipped_frac=float(s[4]) / n, error_min=float(s[5]), error_max=float(s[6]))


# ---- the backward -----------------------------------------------------------------------------------------------------------------------
def backward(sd, x, dvalue, activation):
    """The gradient of L = sum_r dvalue[r] u_r in NumPy fp64, from a VNet state_dict (torch's layout; without a feature_norm the ln0
    gradients are zeros): x [R, 29], dvalue [R] -> a dict of the FIELDS' gradients, and under "z1", "z2" the pre-activations, under "u"
    the forward's raw values"""
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
    c = np.asarray(dvalue, dtype=np.float64).reshape(-1)
    w3 = p["w3"].reshape(H)
    fn = "ln0_g" in p
    if fn:
        n0, rs0 = ln(x)
        xh = n0 * p["ln0_g"] + p["ln0_b"]
    else:
        xh = x
    z1 = xh @ p["w1"].T + p["b1"]
    a1 = act(z1)
    n1, rs1 = ln(a1)
    y1 = n1 * p["ln1_g"] + p["ln1_b"]
    z2 = y1 @ p["w2"].T + p["b2"]
    a2 = act(z2)
    n2, rs2 = ln(a2)
    y2 = n2 * p["ln2_g"] + p["ln2_b"]
    u = y2 @ w3 + p["b3"].reshape(())
    g = {"b3": c.sum(), "w3": c @ y2}
    g["ln2_g"], g["ln2_b"], da2 = ln_back(c[:, None] * w3[None, :], n2, rs2, p["ln2_g"])
    dz2 = da2 * dact(z2, a2)
    g["b2"], g["w2"] = dz2.sum(0), dz2.T @ y1
    g["ln1_g"], g["ln1_b"], da1 = ln_back(dz2 @ p["w2"], n1, rs1, p["ln1_g"])
    dz1 = da1 * dact(z1, a1)
    g["b1"], g["w1"] = dz1.sum(0), dz1.T @ xh
    if fn:
        dxh = dz1 @ p["w1"]
        g["ln0_g"], g["ln0_b"] = (dxh * n0).sum(0), dxh.sum(0)
    else:
        g["ln0_g"], g["ln0_b"] = np.zeros(IN), np.zeros(IN)
    g.update(z1=z1, z2=z2, u=u)
    return g


def flat(g, dtype=np.float64):
    """a dict of the FIELDS' gradients -> [6459] in sdc_critic_params' order"""
    return np.concatenate([np.asarray(g[k], dtype=dtype).reshape(-1) for k in FIELDS])


def split(flat_grads):
    """[6459] -> {field: shaped view}"""
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
    """the workgroups (partials) of sdc_critic_backward for n_rows rows"""
    return min((n_rows + 63) // 64, MAX_BLOCKS)


# ---- torch autograd over a plain-torch network of the same shape (the reference arithmetic the tests measure against) -------------------
def torch_net(sd, activation, dtype=None):
    """a plain torch module with the VNet's parameter names (base.feature_norm, base.mlp.fc.{0,2,3,5}, v_out) holding the state_dict `sd`;
    forward: x [R, 29] -> raw values [R]"""
    import torch
    from torch import nn
    act = nn.Tanh if activation == "tanh" else nn.ReLU
    fn = KEYS["ln0_g"] in sd

    class Mlp(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Sequential(nn.Linear(IN, H), act(), nn.LayerNorm(H), nn.Linear(H, H), act(), nn.LayerNorm(H))

    class Base(nn.Module):
        def __init__(self):
            super().__init__()
            if fn:
                self.feature_norm = nn.LayerNorm(IN)
            self.mlp = Mlp()

        def forward(self, x):
            return self.mlp.fc(self.feature_norm(x) if fn else x)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.base = Base()
            self.v_out = nn.Linear(H, 1)

        def forward(self, x):
            return self.v_out(self.base(x))[..., 0]

    m = Net()
    m.load_state_dict({k: torch.from_numpy(np.array(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()}, strict=True)
    return m.to(dtype) if dtype is not None else m


def torch_value_loss(values, value_preds, returns, scale, shift, clip, delta, flags):
    """v_critic.py cal_value_loss restated in torch, per element (the caller takes the mean): clamp, the Huber masks as constants, the
    binary torch.max; the target (returns - shift) / scale is ValueNorm.normalize"""
    import torch
    clipped = value_preds + (values - value_preds).clamp(-clip, clip)
    t = (returns - shift) / scale
    ec, eo = t - clipped, t - values

    def l(e):
        if not flags & HUBER:
            return e ** 2 / 2
        a = (abs(e) <= delta).to(e.dtype)
        b = (abs(e) > delta).to(e.dtype)
        return a * e ** 2 / 2 + b * delta * (abs(e) - delta / 2)

    lo, lc = l(eo), l(ec)
    return torch.max(lo, lc) if flags & CLIPPED else lo


def _named_grads(net):
    inv = {v: k for k, v in KEYS.items()}
    g = {inv[n]: p.grad.detach().numpy().astype(np.float64).reshape(SHAPES[inv[n]]) for n, p in net.named_parameters()}
    for k in ("ln0_g", "ln0_b"):
        g.setdefault(k, np.zeros(IN))
    return g


def torch_grads(net, x, dvalue):
    """d(sum_r dvalue[r] u_r) / d(parameters) by torch autograd on the CPU in the module's dtype -> {field: fp64 array}"""
    import torch
    dt = next(net.parameters()).dtype
    net.zero_grad()
    u = net(torch.as_tensor(np.asarray(x), dtype=dt))
    (torch.as_tensor(np.asarray(dvalue).reshape(-1), dtype=dt) * u).sum().backward()
    return _named_grads(net)


def torch_loss_grads(net, x, value_preds, returns, scale, shift, clip, delta, flags, coef):
    """d(coef sum_r loss_r) / d(parameters) by torch autograd THROUGH the restated cal_value_loss -> ({field: fp64 array}, the summed loss
    times coef as a float, d loss / d u [R] fp64)"""
    import torch
    dt = next(net.parameters()).dtype
    net.zero_grad()
    T = lambda a: torch.as_tensor(np.asarray(a).reshape(-1), dtype=dt)
    u = net(torch.as_tensor(np.asarray(x), dtype=dt))
    u.retain_grad()
    loss = coef * torch_value_loss(u, T(value_preds), T(returns), scale, shift, clip, delta, flags).sum()
    loss.backward()
    return _named_grads(net), float(loss.detach()), u.grad.detach().numpy().astype(np.float64)
