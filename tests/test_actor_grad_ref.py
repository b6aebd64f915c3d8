"""The NumPy fp64 restatement of the actors' gradient (tests/actor_grad_ref.py) on the CPU: its hand-derived backward against torch fp64
autograd over a plain-torch network of the same shape (agreement at fp64 rounding: observed 0.9e-15 to 4.0e-15 under the measure below, at
67 and at 3001 rows), and against the gradients the reference's own HAPPO.update left in fp32 (tests/golden/actor_grad/actor_grad.npz)
under the measure max|delta| / max|g| per parameter tensor with the bar 1e-5 (torch fp32 against torch fp64 on networks of this shape:
6e-7 to 2.3e-6; DESIGN.md section 4.28 records what this test observes); the dlogp rule against torch autograd of min and clamp at the
tie cases; the ordered sum of squares against a plain sum.  No GPU."""
import numpy as np
import pytest

from tests import actor_grad_ref as GR

FIXTURE_BAR = 1e-5
FP64_BAR = 1e-11      # fp64 rounding through sums of a few thousand terms and two LayerNorms (observed: 4e-15 at most)


def _inputs(rows, seed, fixture_obs):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, 26)).astype(np.float32)
    x[1::3, 14:] = 0.0
    x[2::3, 13:] = 0.0
    x[:min(rows, len(fixture_obs))] = fixture_obs[:rows]
    actions = rng.integers(0, 3, size=rows).astype(np.int32)
    coef = (rng.standard_normal(rows) / rows).astype(np.float32)
    coef[::7] = 0.0
    return x, actions, coef, -0.01 / rows


@pytest.mark.parametrize("rows", [67, 3001])
@pytest.mark.parametrize("activation,feature_norm", GR.CONFIGS)
def test_backward_is_torch_fp64_autograd(activation, feature_norm, rows):
    import torch
    c = GR.case(activation, feature_norm)
    x, actions, coef, dent = _inputs(rows, 500 + rows, c["obs"])
    g = GR.backward(c["sd"], x, actions, coef, dent, activation)
    want = GR.torch_grads(GR.torch_net(c["sd"], activation, torch.float64), x, actions, coef, dent)
    dist = GR.distance(g, want)
    print(GR.cfg_name(activation, feature_norm), rows, "rows: restatement against torch fp64 autograd, worst %.2e" % max(dist.values()))
    assert max(dist.values()) <= FP64_BAR, dist
    if not feature_norm:
        assert not g["ln0_gamma"].any() and not g["ln0_beta"].any()
    assert GR.flat(g).shape == (GR.N_PARAMS,) and GR.N_PARAMS == 6391


@pytest.mark.parametrize("activation,feature_norm", GR.CONFIGS)
def test_backward_gives_the_references_gradients(activation, feature_norm):
    """the whole chain -- forward, log-probabilities, the dlogp rule, the backward -- against every .grad HAPPO.update left"""
    c = GR.case(activation, feature_norm)
    fx = GR.fixture()
    clip, coef_ent = float(fx["clip_param"]), float(fx["entropy_coef"])
    assert c["actor_grad_norm"] < fx["max_grad_norm"] and c["ratio_margin"] > 1e-4                  # (unclipped; no ratio near a clip edge)
    assert activation != "relu" or c["relu_margin"] > 1e-5
    fwd = GR.backward(c["sd"], c["obs"], c["actions"], np.zeros(GR.R), 0.0, activation)
    lg = fwd["logits"]
    zc = lg - lg.max(-1, keepdims=True)
    logp = zc - np.log(np.exp(zc).sum(-1, keepdims=True))
    new = np.take_along_axis(logp, c["actions"].astype(np.int64), -1)                                # [R, 1]
    _, r, _, d = GR.dlogp(np.repeat(new, 3, -1), np.repeat(c["old_log_probs"], 3, -1), c["advantages"][:, 0], 0, clip,
                          factor=c["factor"][:, 0], scale=1.0 / GR.R, fp32_inputs=False)
    assert np.minimum(np.abs(r - (1 - clip)), np.abs(r - (1 + clip))).min() > 1e-4      # (the fp64 ratios take the reference's branches)
    g = GR.backward(c["sd"], c["obs"], c["actions"], d, -coef_ent / GR.R, activation)
    if activation == "relu":
        assert GR.relu_margin(g) > 1e-5
    want = {k: c["grad"][v] for k, v in GR.KEYS.items() if v in c["grad"]}
    for k in ("ln0_gamma", "ln0_beta"):
        want.setdefault(k, np.zeros(26, np.float32))
    dist = GR.distance(g, want)
    print(GR.cfg_name(activation, feature_norm), "restatement against the reference's fp32 gradients: worst %.2e (%s)" % (
        max(dist.values()), max(dist, key=dist.get)))
    assert max(dist.values()) <= FIXTURE_BAR, dist
    norm = np.sqrt((GR.flat(g) ** 2).sum())
    assert abs(norm - float(c["actor_grad_norm"])) <= 1e-5 * norm


# (r, A) of the issue's tie cases, clip 0.2: r = 1; r exactly on a bound; r = 1.2 (the upper bound as 1 + 0.2 forms it); r inside and outside
TIES = [(1.0, 2.0), (1.0, 0.0), (1.0 - 0.2, 2.0), (1.0 - 0.2, -1.0), (1.0 + 0.2, 2.0), (1.2, 2.0), (0.5, 2.0), (0.5, -2.0), (1.5, 2.0), (1.5, -2.0)]


def test_dlogp_rule_is_what_torch_differentiates_at_the_ties():
    import torch
    clip, scale, F = 0.2, 0.125, 1.3
    r = np.array([t[0] for t in TIES])
    A = np.array([t[1] for t in TIES])
    d, is_open = GR.dlogp_rule(r, A, np.full(len(TIES), F), scale, clip)
    logp = torch.zeros(len(TIES), dtype=torch.float64, requires_grad=True)
    rt = torch.as_tensor(r) * torch.exp(logp)                    # (d r / d logp = r at logp = 0)
    At = torch.as_tensor(A)
    loss = -(scale * F * torch.min(rt * At, torch.clamp(rt, 1.0 - clip, 1.0 + clip) * At)).sum()
    loss.backward()
    want = logp.grad.numpy()
    assert np.allclose(d, want, rtol=1e-15, atol=0.0), (d, want)
    # the rule's branches: inside and on the bounds open; below with A > 0 and above with A < 0 open; the other two closed
    assert list(is_open) == [True, True, True, True, True, True, True, False, False, True]
    assert d[1] == 0.0 and d[7] == 0.0 and d[8] == 0.0


def test_dlogp_reads_the_agents_column_and_rounds_once():
    rng = np.random.default_rng(3)
    new = rng.standard_normal((5, 7, 3)).astype(np.float32) * 0.2
    old = rng.standard_normal((5, 7, 3)).astype(np.float32) * 0.2
    old[0, :3] = new[0, :3]
    adv = rng.standard_normal((5, 7)).astype(np.float32)
    for agent in range(3):
        poisoned = new.copy()
        poisoned[..., [a for a in range(3) if a != agent]] = np.nan
        d32, r, is_open, d64 = GR.dlogp(poisoned, old, adv, agent, 0.2)
        assert d32.dtype == np.float32 and np.isfinite(d32).all() and np.array_equal(d32, d64.astype(np.float32))
        assert (r[0, :3] == 1.0).all() and np.array_equal(d32[0, :3], (-(adv[0, :3].astype(np.float64) / 35.0)).astype(np.float32))


def test_grad_sq_order():
    rng = np.random.default_rng(11)
    g = rng.standard_normal(GR.N_PARAMS).astype(np.float32)
    s = GR.grad_sq(g)
    plain = float((g.astype(np.float64) ** 2).sum())
    assert abs(s - plain) <= 1e-12 * plain
    assert GR.grad_sq(np.zeros(GR.N_PARAMS, np.float32)) == 0.0
    one = np.zeros(GR.N_PARAMS, np.float32)
    one[6390] = 3.0
    assert GR.grad_sq(one) == 9.0
    assert GR.blocks(1) == 1 and GR.blocks(64) == 1 and GR.blocks(65) == 2 and GR.blocks(10 ** 6) == GR.MAX_BLOCKS
