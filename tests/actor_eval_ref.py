"""What the tests of sdc_actor_evaluate share (TEST INFRASTRUCTURE, never imported by the product): the fixture the reference wrote
(tests/golden/actor_eval/actor_eval.npz, tests/golden/gen_actor_eval_golden.py), its networks as state_dicts and as torch modules, a
NumPy fp64 forward of the network in torch's layout, and the kernel's packed layout (csrc/sdc_actor_eval_pack.hpp SdcActorEvalDev) read
from its bytes, un-permuted, and run forward in NumPy fp64 in the kernel's data flow.  A plain module: no GPU."""
import functools
import os

import numpy as np

from tests.critic_ref import unit_of_k

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "actor_eval", "actor_eval.npz")
CONFIGS = [("tanh", True), ("tanh", False), ("relu", True), ("relu", False)]
R = 67
IN, H, OUT, S1, EPS = 26, 64, 3, 7, 1e-5
KEYS = {"ln0_gamma": "base.feature_norm.weight", "ln0_beta": "base.feature_norm.bias",
        "w1": "base.mlp.fc.0.weight", "b1": "base.mlp.fc.0.bias", "ln1_gamma": "base.mlp.fc.2.weight", "ln1_beta": "base.mlp.fc.2.bias",
        "w2": "base.mlp.fc.3.weight", "b2": "base.mlp.fc.3.bias", "ln2_gamma": "base.mlp.fc.5.weight", "ln2_beta": "base.mlp.fc.5.bias",
        "w3": "act.action_out.linear.weight", "b3": "act.action_out.linear.bias"}


def cfg_name(activation, feature_norm):
    return "%s_fn%d" % (activation, int(feature_norm))


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def case(activation, feature_norm):
    """one configuration's arrays without their prefix, its state_dict under "sd" """
    c = cfg_name(activation, feature_norm) + "_"
    out = {k[len(c):]: v for k, v in fixture().items() if k.startswith(c)}
    out["sd"] = {k[len("sd_"):]: v for k, v in out.items() if k.startswith("sd_")}
    return out


def params(activation, feature_norm):
    """what SdcEngine.set_actor / engine.actor_params take"""
    return dict(case(activation, feature_norm)["sd"], activation=activation)


def torch_net(activation, feature_norm, dtype=None):
    """tests/actor_ref.torch_actor holding the configuration's parameters"""
    import torch
    from tests import actor_ref as AR
    m = AR.torch_actor(1, activation, feature_norm=feature_norm)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in case(activation, feature_norm)["sd"].items()}, strict=True)
    return m.to(dtype) if dtype is not None else m


def forward(sd, x, activation):
    """x [..., 26] -> logits [..., 3] in NumPy fp64 from a state_dict (torch's layout)"""
    p = {k: np.asarray(sd[v], dtype=np.float64) for k, v in KEYS.items() if v in sd}
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))

    def ln(h, g, b):
        mean = h.mean(-1, keepdims=True)
        var = ((h - mean) ** 2).mean(-1, keepdims=True)
        return (h - mean) / np.sqrt(var + EPS) * g + b

    h = np.asarray(x, dtype=np.float64)
    if "ln0_gamma" in p:
        h = ln(h, p["ln0_gamma"], p["ln0_beta"])
    h = ln(act(h @ p["w1"].T + p["b1"]), p["ln1_gamma"], p["ln1_beta"])
    h = ln(act(h @ p["w2"].T + p["b2"]), p["ln2_gamma"], p["ln2_beta"])
    return h @ p["w3"].T + p["b3"]


# ---- the kernel's packed layout, read from its bytes -----------------------------------------------------------------------------------
LAYOUT = (("a1", (S1, 64, 4)), ("a2", (16, 64, 4)), ("ln0_g", (4, 8)), ("ln0_b", (4, 8)), ("b1", (4, 4, 4)), ("ln1_g", (4, 4, 4)),
          ("ln1_b", (4, 4, 4)), ("b2", (4, 4, 4)), ("ln2_g", (4, 4, 4)), ("ln2_b", (4, 4, 4)), ("w3", (OUT, 4, 4, 4)), ("b3", (4,)))
PACKED_FLOATS = sum(int(np.prod(s)) for _, s in LAYOUT)
PACKED_BYTES = 4 * (PACKED_FLOATS + 4)          # (flags and three ints of padding)


def parse_packed(raw: bytes):
    assert len(raw) == PACKED_BYTES, len(raw)
    f = np.frombuffer(raw, dtype=np.float32)
    d, at = {}, 0
    for name, shape in LAYOUT:
        n = int(np.prod(shape, dtype=np.int64))
        d[name] = f[at:at + n].reshape(shape).copy()
        at += n
    ints = np.frombuffer(raw, dtype=np.int32)[at:]
    d["flags"] = int(ints[0])
    assert not ints[1:].any()
    return d


def unpack(d):
    """the packed layout -> torch's: w1 [64, 28], w2 [64, 64], w3 [3, 64], the per-unit vectors [64], ln0 [32]; the padding included"""
    out = {"w1": np.zeros((H, 4 * S1), np.float32), "w2": np.zeros((H, H), np.float32), "w3": np.zeros((OUT, H), np.float32)}
    for l in range(64):
        g, e = l >> 4, l & 15
        for t in range(4):
            for s in range(S1):
                out["w1"][16 * t + e, 4 * s + g] = d["a1"][s, l, t]
            for s in range(16):
                out["w2"][16 * t + e, unit_of_k(4 * s + g)] = d["a2"][s, l, t]
    for name in ("b1", "ln1_g", "ln1_b", "b2", "ln2_g", "ln2_b"):
        out[name] = np.zeros(H, np.float32)
    for g in range(4):
        for t in range(4):
            for i in range(4):
                u = 16 * t + 4 * g + i
                for name in ("b1", "ln1_g", "ln1_b", "b2", "ln2_g", "ln2_b"):
                    out[name][u] = d[name][g, t, i]
                out["w3"][:, u] = d["w3"][:, g, t, i]
    for name in ("ln0_g", "ln0_b"):
        v = np.zeros(32, np.float32)
        for g in range(4):
            for s in range(8):
                v[4 * s + g] = d[name][g, s]
        out[name] = v
    out["b3"] = d["b3"].copy()
    return out


def packed_forward(d, x, activation):
    """x [16, 26] -> logits [16, 3] in NumPy fp64 from the packed layout, in the kernel's data flow (one wavefront's 16 rows)"""
    d = {k: (np.asarray(v, dtype=np.float64) if k != "flags" else v) for k, v in d.items()}
    act = np.tanh if activation == "tanh" else (lambda v: np.maximum(v, 0.0))
    xp = np.zeros((16, 4 * S1))
    xp[:, :IN] = np.asarray(x, dtype=np.float64)
    lanes = np.arange(64)
    G, E = lanes >> 4, lanes & 15
    xs = np.stack([xp[E, 4 * s + G] for s in range(S1)])                     # the B operands: lane (g, e) holds entry 4 s + g of row e
    if d["flags"] & 1:
        mean = xp.sum(-1) / IN
        var = (xp ** 2).sum(-1) / IN - mean ** 2
        rs = 1.0 / np.sqrt(var + EPS)
        xs = np.stack([(xs[s] - mean[E]) * rs[E] * d["ln0_g"][G, s] + d["ln0_b"][G, s] for s in range(S1)])

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
    out = np.zeros((16, OUT))
    for c in range(OUT):
        part = (d["w3"][c][G] * h2).sum((1, 2))
        np.add.at(out[:, c], E, part)
        out[:, c] += d["b3"][c]
    return out
