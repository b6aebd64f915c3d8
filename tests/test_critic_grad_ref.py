"""The NumPy fp64 restatement of the critic's gradient (tests/critic_grad_ref.py) on the CPU: its hand-derived backward and its value-loss
rule against torch fp64 autograd of a plain-torch network and of cal_value_loss restated in torch (agreement at fp64 rounding under the
measure max|delta| / max|g| per parameter tensor, bar 1e-12: sums of a few thousand fp64 terms; observed 1.7e-15 to 5.5e-14 at 67 and
at 3001 rows), the loss rule against autograd at every tie and edge -- exact inputs, clip 0.25, multiples of 1/8 --, and the whole chain
against the gradients the reference's own VCritic.update left in fp32 (tests/golden/critic_grad/critic_grad.npz) with the project's bar
1e-5 (observed: 3.7e-7 to 1.8e-6 over the eight cases, the loss to 2.0e-7, the norm to 8.1e-8); the ordered sum of squares and the
ordered statistics against plain sums.  No GPU."""
import numpy as np
import pytest

from tests import critic_grad_ref as GR
from dc_rl_amd.engine import value_norm_scale_shift

FIXTURE_BAR = 1e-5
FP64_BAR = 1e-12
LOSS_FLAGS = {"huber_clip": GR.HUBER | GR.CLIPPED, "mse": 0}


def _inputs(rows, seed, fixture_rows):
    """rows of share_obs (the fixture's first), stored predictions on both sides of the clip, returns whose errors straddle delta"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, 29)).astype(np.float32)
    x[1::3, 20:] = 0.0
    x[:min(rows, len(fixture_rows))] = fixture_rows[:rows]
    return x, rng


@pytest.mark.parametrize("rows", [67, 3001])
@pytest.mark.parametrize("activation,feature_norm", GR.CONFIGS)
def test_backward_and_loss_are_torch_fp64_autograd(activation, feature_norm, rows):
    import torch
    c = GR.case(activation, feature_norm)
    x, rng = _inputs(rows, 700 + rows, c["share_obs"])
    # 1. the backward alone, under arbitrary coefficients
    coef = (rng.standard_normal(rows) / rows).astype(np.float32)
    coef[::7] = 0.0
    g = GR.backward(c["sd"], x, coef, activation)
    net = GR.torch_net(c["sd"], activation, torch.float64)
    want = GR.torch_grads(net, x, coef)
    dist = GR.distance(g, want)
    worst = max(dist.values())
    assert worst <= FP64_BAR, dist
    if not feature_norm:
        assert not g["ln0_g"].any() and not g["ln0_b"].any()
    assert GR.flat(g).shape == (GR.N_PARAMS,) and GR.N_PARAMS == 6459
    # 2. the chain through the loss, for the four flag combinations: u in fp64, the rule, the backward
    u = g["u"]
    gap = np.where(rng.random(rows) < 0.5, rng.uniform(0.25, 0.6, rows), rng.uniform(0.01, 0.15, rows)) * rng.choice([-1.0, 1.0], rows)
    vp = (u + gap).astype(np.float32)
    ret = (40.0 + 12.0 * (u + 1.2 * rng.standard_normal(rows))).astype(np.float32)
    scale, shift, clip, delta = 11.5, 40.25, 0.2, 1.0
    for flags in (0, 1, 2, 3):
        v = GR.value_loss(u, vp, ret, scale, shift, clip, delta, flags, 1.0 / rows)
        if flags & GR.CLIPPED:      # (away from the branch points, where fp64 rounding could choose another side than torch)
            assert np.abs(np.abs(v["d"]) - clip).min() > 1e-9 and np.abs(v["lo"] - v["lc"])[np.abs(v["d"]) > clip].min() > 1e-12
        if flags & GR.HUBER:
            assert min(np.abs(np.abs(v["eo"]) - delta).min(), np.abs(np.abs(v["ec"]) - delta).min()) > 1e-9
            assert (np.abs(v["eo"]) > delta).sum() > 5 and (np.abs(v["eo"]) <= delta).sum() > 5
        gl = GR.backward(c["sd"], x, v["g"] / rows, activation)
        want, loss, du = GR.torch_loss_grads(net, x, vp, ret, scale, shift, clip, delta, flags, 1.0 / rows)
        assert np.abs(v["g"] / rows - du).max() <= 1e-14 * np.abs(du).max()      # (a handful of fp64 roundings: / rows here, * (1 / rows) there)
        assert abs(v["L"].sum() / rows - loss) <= 1e-13 * abs(loss)
        d2 = max(GR.distance(gl, want).values())
        worst = max(worst, d2)
        assert d2 <= FP64_BAR, (flags, GR.distance(gl, want))
    print(GR.cfg_name(activation, feature_norm), rows, "rows: restatement against torch fp64 autograd, worst %.2e" % worst)


# (u, vp, t) at clip 0.25, delta 1, scale 1, shift 0: every tie and edge of the rule, all exact in binary
TIES = [
    (0.5, 0.25, 0.75),      # d = +clip exactly: the clamp passes the gradient, l(eo) = l(ec)
    (0.25, 0.5, 0.75),      # d = -clip exactly
    (0.5, 0.25, 2.0),       # ... in the Huber loss's linear regime
    (0.5, 0.5, 1.5),        # eo = +delta
    (0.5, 0.5, -0.5),       # eo = -delta
    (1.0, 0.0, 1.25),       # d outside, ec = +delta, eo inside
    (0.125, 0.0, 0.5),      # l(eo) = l(ec) with d inside (uc = u)
    (1.0, 0.0, 0.625),      # l(eo) = l(ec) with d outside: eo = -0.375, ec = +0.375
    (4.25, 0.0, 2.25),      # ... both in the linear regime: eo = -2, ec = +2
    (-1.0, 0.0, -0.625),    # ... on the lower side
    (0.5, 0.5, 0.5),        # e = 0, d = 0
    (1.0, 0.0, 1.0),        # eo = 0 with d outside: the clipped loss is the larger, no gradient
    (1.0, 0.0, 0.25),       # ec = 0 with d outside: the original loss is the larger
    (0.375, 0.25, 3.0),     # plain cases: inside, original larger / clipped larger, outside on both sides
    (2.0, 0.0, 3.0), (2.0, 0.0, -1.0), (-2.0, 0.0, 3.0), (-2.0, 0.0, -3.0),
]


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_loss_rule_is_what_torch_differentiates_at_every_tie_and_edge(flags):
    import torch
    clip, delta, coef = 0.25, 1.0, 0.5
    u, vp, t = (np.array([c[i] for c in TIES]) for i in range(3))
    v = GR.value_loss(u, vp, t, 1.0, 0.0, clip, delta, flags, coef)
    ut = torch.tensor(u, dtype=torch.float64, requires_grad=True)
    loss = GR.torch_value_loss(ut, torch.tensor(vp), torch.tensor(t), 1.0, 0.0, clip, delta, flags)
    (coef * loss).sum().backward()
    assert np.array_equal(v["L"], loss.detach().numpy()), (v["L"], loss)
    assert np.array_equal(coef * v["g"], ut.grad.numpy()), (coef * v["g"], ut.grad)      # (-0.0 == 0.0)
    assert np.array_equal(v["dvalue"], (coef * v["g"]).astype(np.float32)) and v["loss"].dtype == v["dvalue"].dtype == np.float32
    # the cases are what they say they are
    assert v["d"][0] == clip and v["d"][1] == -clip and v["eo"][3] == delta and v["eo"][4] == -delta and v["ec"][5] == delta
    for i in (0, 1, 2, 6, 7, 8, 9, 10):
        assert v["lo"][i] == v["lc"][i], i
    assert v["eo"][10] == 0.0 and v["eo"][11] == 0.0 and v["ec"][12] == 0.0
    if flags & GR.CLIPPED:
        assert v["g"][7] == 0.5 * 0.375 and v["g"][11] == 0.0 and v["g"][0] == -0.25      # a halved tie; no gradient; the clamp's edge passes


@pytest.mark.parametrize("loss_name", ["huber_clip", "mse"])
@pytest.mark.parametrize("activation,feature_norm", GR.CONFIGS)
def test_the_chain_gives_the_references_gradients(activation, feature_norm, loss_name):
    """forward, ValueNorm.normalize, the loss rule, the backward -- against every .grad VCritic.update left, its loss and its norm"""
    c = GR.case(activation, feature_norm, loss_name)
    fx = GR.fixture()
    clip, delta, coef = float(fx["clip_param"]), float(fx["huber_delta"]), float(fx["value_loss_coef"])
    flags = LOSS_FLAGS[loss_name]
    assert c["critic_grad_norm"] < fx["max_grad_norm"] and c["clip_margin"] > 1e-4
    assert activation != "relu" or c["relu_margin"] > 1e-5
    scale, shift = value_norm_scale_shift((c["norm_mean"], c["norm_var"]))
    u = GR.backward(c["sd"], c["share_obs"], np.zeros(GR.R), activation)["u"]
    v = GR.value_loss(u, c["value_preds"][:, 0], c["returns"][:, 0], scale, shift, clip, delta, flags, coef / GR.R)
    # the fp64 terms take the reference's fp32 branches
    assert np.abs(np.abs(v["d"]) - clip).min() > 1e-4
    if flags & GR.HUBER:
        assert min(np.abs(np.abs(v["eo"]) - delta).min(), np.abs(np.abs(v["ec"]) - delta).min()) > 1e-4
        assert (np.abs(v["eo"]) > delta).sum() >= 10 and (np.abs(v["eo"]) <= delta).sum() >= 10
    if flags & GR.CLIPPED:
        outside = np.abs(v["d"]) > clip
        assert np.abs(v["lo"] - v["lc"])[outside].min() > 1e-6 and outside.sum() >= 10 and (~outside).sum() >= 10
    g = GR.backward(c["sd"], c["share_obs"], (coef / GR.R) * v["g"], activation)
    if activation == "relu":
        assert GR.relu_margin(g) > 1e-5
    want = {k: c["grad"][key].reshape(GR.SHAPES[k]) for k, key in GR.KEYS.items() if key in c["grad"]}
    for k in ("ln0_g", "ln0_b"):
        want.setdefault(k, np.zeros(29, np.float32))
    dist = GR.distance(g, want)
    loss = v["L"].mean()
    norm = np.sqrt((GR.flat(g) ** 2).sum())
    print("%s %s: restatement against the reference's fp32 gradients: worst %.2e (%s), loss %.2e, norm %.2e" % (
        GR.cfg_name(activation, feature_norm), loss_name, max(dist.values()), max(dist, key=dist.get),
        abs(loss - float(c["value_loss"])) / loss, abs(norm - float(c["critic_grad_norm"])) / norm))
    assert max(dist.values()) <= FIXTURE_BAR, dist
    assert abs(loss - float(c["value_loss"])) <= FIXTURE_BAR * loss
    assert abs(norm - float(c["critic_grad_norm"])) <= FIXTURE_BAR * norm


def test_grad_sq_and_stats_order():
    rng = np.random.default_rng(11)
    g = rng.standard_normal(GR.N_PARAMS).astype(np.float32)
    s = GR.grad_sq(g)
    plain = float((g.astype(np.float64) ** 2).sum())
    assert abs(s - plain) <= 1e-12 * plain
    assert GR.grad_sq(np.zeros(GR.N_PARAMS, np.float32)) == 0.0
    one = np.zeros(GR.N_PARAMS, np.float32)
    one[6458] = 3.0
    assert GR.grad_sq(one) == 9.0
    assert GR.blocks(1) == 1 and GR.blocks(64) == 1 and GR.blocks(65) == 2 and GR.blocks(10 ** 6) == GR.MAX_BLOCKS
    n = 1480
    u, vp, ret = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    v = GR.value_loss(u, vp, ret, 1.5, 0.25, 0.2, 1.0, 3, 1.0 / n)
    st = GR.stats(v)
    assert st[7] == n and st[4] == (v["lc"] > v["lo"]).sum() and st[5] == v["eo"].min() and st[6] == v["eo"].max()
    assert abs(st[0] - v["loss"].astype(np.float64).sum()) <= 1e-12 * st[0] and abs(st[3] - (v["eo"] ** 2).sum()) <= 1e-12 * st[3]
    sm = GR.summary(st)
    assert abs(sm["value_loss"] - v["loss"].mean()) <= 1e-6 and 0.0 < sm["clipped_frac"] < 1.0 and sm["error_min"] < sm["error_mean"] < sm["error_max"]
