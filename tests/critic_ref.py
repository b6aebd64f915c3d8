"""Tests-only restatement of the V critic (TEST INFRASTRUCTURE, never imported by the product): the reference's VNet
(harl/models/value_function_models/v_net.py over harl/models/base/mlp.py MLPBase, hidden_sizes [64, 64], no recurrence) and
ValueNorm.denormalize (harl/common/valuenorm.py), written from their definition in torch, fp64 by default:

    LayerNorm(29) [use_feature_normalization] -> Linear(29, 64) -> act -> LayerNorm(64) -> Linear(64, 64) -> act -> LayerNorm(64)
    -> Linear(64, 1);  v * sqrt(var) + mean

LayerNorm: biased variance, eps 1e-5, (x - mean) / sqrt(var + eps) * gain + bias.

  * `make_critic` -- a seeded VNet state_dict: torch's default Linear init (weights and biases uniform in +-1 / sqrt(fan_in)), every
                     LayerNorm gain 1 + 0.2 N(0, 1) and bias 0.2 N(0, 1), so that a swapped gain / bias or a wrong unit order shows.
  * `forward`     -- the restatement, in `dtype` (fp64: the yardstick; fp32: torch's own distance from it on the same rows).
  * `packed_forward` -- the same network computed in NumPy fp64 FROM THE KERNELS' PACKED LAYOUT (csrc/sdc_critic_pack.hpp), in the
                     kernels' data flow: lane (g, e), accumulator (t, i), layer 2's k-step 4 t + i reading register (t, i).
  * `unpack`      -- the packed layout back to torch's.
"""
from __future__ import annotations

import numpy as np

IN, H = 29, 64
EPS = 1e-5
KEYS = {"w1": "base.mlp.fc.0.weight", "b1": "base.mlp.fc.0.bias", "ln1_g": "base.mlp.fc.2.weight", "ln1_b": "base.mlp.fc.2.bias",
        "w2": "base.mlp.fc.3.weight", "b2": "base.mlp.fc.3.bias", "ln2_g": "base.mlp.fc.5.weight", "ln2_b": "base.mlp.fc.5.bias",
        "w3": "v_out.weight", "b3": "v_out.bias", "ln0_g": "base.feature_norm.weight", "ln0_b": "base.feature_norm.bias"}
VALUE_NORM = (-3.0, 7.5 ** 2)      # (mean, var): scale 7.5, shift -3


def make_critic(seed, feature_norm=True):
    """-> a VNet state_dict of fp32 torch tensors (no base.feature_norm.* with feature_norm False)"""
    import torch
    g = torch.Generator().manual_seed(seed)

    def linear(out, inp):
        bound = 1.0 / np.sqrt(inp)
        return ((torch.rand((out, inp), generator=g) * 2 - 1) * bound, (torch.rand((out,), generator=g) * 2 - 1) * bound)

    def norm(n):
        return 1.0 + 0.2 * torch.randn((n,), generator=g), 0.2 * torch.randn((n,), generator=g)

    sd = {}
    n0 = norm(IN)
    if feature_norm:
        sd[KEYS["ln0_g"]], sd[KEYS["ln0_b"]] = n0
    sd[KEYS["w1"]], sd[KEYS["b1"]] = linear(H, IN)
    sd[KEYS["ln1_g"]], sd[KEYS["ln1_b"]] = norm(H)
    sd[KEYS["w2"]], sd[KEYS["b2"]] = linear(H, H)
    sd[KEYS["ln2_g"]], sd[KEYS["ln2_b"]] = norm(H)
    sd[KEYS["w3"]], sd[KEYS["b3"]] = linear(1, H)
    return {k: v.float().contiguous() for k, v in sd.items()}


def _layer_norm(x, gain, bias):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / (var + EPS).sqrt() * gain + bias


def forward(sd, x, activation="tanh", value_norm=None, dtype=None):
    """x [..., 29] (any float tensor, on the CPU) -> values [...] in `dtype` (default fp64); value_norm: None or (mean, var)"""
    import torch
    dtype = dtype or torch.float64
    p = {k: sd[v].detach().cpu().to(dtype) for k, v in KEYS.items() if v in sd}
    act = torch.tanh if activation == "tanh" else torch.relu
    h = x.detach().cpu().to(dtype)
    if "ln0_g" in p:
        h = _layer_norm(h, p["ln0_g"], p["ln0_b"])
    h = _layer_norm(act(h @ p["w1"].T + p["b1"]), p["ln1_g"], p["ln1_b"])
    h = _layer_norm(act(h @ p["w2"].T + p["b2"]), p["ln2_g"], p["ln2_b"])
    v = (h @ p["w3"].T + p["b3"])[..., 0]
    if value_norm is not None:
        mean, var = value_norm
        v = v * torch.tensor(var, dtype=dtype).sqrt() + torch.tensor(mean, dtype=dtype)
    return v


# ---- the kernels' packed layout (csrc/sdc_critic_pack.hpp SdcCriticDev), read from its bytes ------------------------------------------
PACKED_FLOATS = 8 * 64 * 4 + 16 * 64 * 4 + 2 * 32 + 7 * 64 + 3
PACKED_BYTES = 4 * (PACKED_FLOATS + 1)


def parse_packed(raw: bytes):
    assert len(raw) == PACKED_BYTES, len(raw)
    f = np.frombuffer(raw, dtype=np.float32)
    d, at = {}, 0
    for name, shape in (("a1", (8, 64, 4)), ("a2", (16, 64, 4)), ("ln0_g", (4, 8)), ("ln0_b", (4, 8)), ("b1", (4, 4, 4)),
                        ("ln1_g", (4, 4, 4)), ("ln1_b", (4, 4, 4)), ("b2", (4, 4, 4)), ("ln2_g", (4, 4, 4)), ("ln2_b", (4, 4, 4)),
                        ("w3", (4, 4, 4)), ("b3", ()), ("scale", ()), ("shift", ())):
        n = int(np.prod(shape, dtype=np.int64))
        d[name] = f[at:at + n].reshape(shape).copy()
        at += n
    d["flags"] = int(np.frombuffer(raw, dtype=np.int32)[at])
    assert at == PACKED_FLOATS
    return d


def unit_of_k(k):
    """layer 2's k index 16 t + 4 i + g -> the hidden unit 16 t + 4 g + i it stands for"""
    return (k & 0x30) | ((k & 3) << 2) | ((k >> 2) & 3)


def unpack(d):
    """the packed layout -> torch's: w1 [64, 29], w2 [64, 64], the per-unit vectors [64], ln0 [29]; and what the padding holds"""
    out = {"w1": np.zeros((H, 32), np.float32), "w2": np.zeros((H, H), np.float32)}
    for l in range(64):
        g, e = l >> 4, l & 15
        for t in range(4):
            for s in range(8):
                out["w1"][16 * t + e, 4 * s + g] = d["a1"][s, l, t]
            for s in range(16):
                out["w2"][16 * t + e, unit_of_k(4 * s + g)] = d["a2"][s, l, t]
    for name in ("b1", "ln1_g", "ln1_b", "b2", "ln2_g", "ln2_b", "w3"):
        v = np.zeros(H, np.float32)
        for g in range(4):
            for t in range(4):
                for i in range(4):
                    v[16 * t + 4 * g + i] = d[name][g, t, i]
        out[name] = v
    for name in ("ln0_g", "ln0_b"):
        v = np.zeros(32, np.float32)
        for g in range(4):
            for s in range(8):
                v[4 * s + g] = d[name][g, s]
        out[name] = v
    return out


def packed_forward(d, x, activation):
    """x [16, 29] -> values [16] in NumPy fp64 from the packed layout, in the kernels' data flow (one wavefront's 16 rows)"""
    d = {k: (np.asarray(v, dtype=np.float64) if k != "flags" else v) for k, v in d.items()}
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    xp = np.zeros((16, 32))
    xp[:, :IN] = np.asarray(x, dtype=np.float64)
    lanes = np.arange(64)
    G, E = lanes >> 4, lanes & 15
    # the B operands: lane (g, e) holds entry 4 s + g of row e
    xs = np.stack([xp[E, 4 * s + G] for s in range(8)])                      # [8, 64]
    if d["flags"] & 1:
        mean = xp.sum(-1) / IN
        var = (xp ** 2).sum(-1) / IN - mean ** 2
        rs = 1.0 / np.sqrt(var + EPS)
        xs = np.stack([(xs[s] - mean[E]) * rs[E] * d["ln0_g"][G, s] + d["ln0_b"][G, s] for s in range(8)])

    def mfma(acc, a, b):
        """D[i][j] += sum_k A[i][k] B[k][j], lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], holds D[4 g + r][e]"""
        A = np.zeros((16, 4))
        B = np.zeros((4, 16))
        A[E, G] = a
        B[G, E] = b
        D = A @ B
        return acc + np.stack([D[4 * G + r, E] for r in range(4)], -1)      # [64, 4]

    def layer(a_op, b_ops, bias, gain, beta):
        acc = [d[bias][G, t, :].copy() for t in range(4)]                    # [4][64 lanes, 4 registers]
        for s, b in enumerate(b_ops):
            for t in range(4):
                acc[t] = mfma(acc[t], d[a_op][s, :, t], b)
        v = act(np.stack(acc, 1))                                            # [64, t, i]
        tot = np.zeros(16)
        sq = np.zeros(16)
        np.add.at(tot, E, v.sum((1, 2)))
        mean = tot / H
        np.add.at(sq, E, ((v - mean[E, None, None]) ** 2).sum((1, 2)))
        rs = 1.0 / np.sqrt(sq / H + EPS)
        return (v - mean[E, None, None]) * rs[E, None, None] * d[gain][G] + d[beta][G]

    h1 = layer("a1", list(xs), "b1", "ln1_g", "ln1_b")
    h2 = layer("a2", [h1[:, s >> 2, s & 3] for s in range(16)], "b2", "ln2_g", "ln2_b")
    part = (d["w3"][G] * h2).sum((1, 2))
    v = np.zeros(16)
    np.add.at(v, E, part)
    return (v + d["b3"]) * d["scale"] + d["shift"]
