"""The restatement chain against the fixture the reference wrote (tests/golden/optim/optim.npz, tests/golden/gen_optim_golden.py): three
consecutive updates, each the gradient of tests/actor_grad_ref.py / tests/critic_grad_ref.py (fp64, rounded once to the fp32 a device
gradient is) followed by the step of tests/optim_ref.py, on the inputs of the existing gradient fixtures.  The reference's fp64 results
are the truth; the chain's largest distance to them may be at most 8 times the distance of the reference's own fp32 results -- the bar
the gradient tests use, and this chain consumes those gradients.  DESIGN.md section 4.31 records what this prints.  No GPU."""
import numpy as np

from dc_rl_amd.engine import value_norm_scale_shift
from tests import actor_grad_ref as AG
from tests import critic_grad_ref as CG
from tests import optim_ref as O

MARGIN = 8.0


def test_fixture_is_data_only_and_small():
    import os
    fx = O.fixture()
    assert os.path.getsize(O.FIXTURE) <= os.path.getsize(CG.FIXTURE)
    assert all(v.dtype.kind in "fU" for v in fx.values()), {k: v.dtype for k, v in fx.items()}
    for u in range(1, O.UPDATES + 1):
        assert fx["actor_p32_%d" % u].dtype == np.float32 and fx["actor_p64_%d" % u].dtype == np.float64
        assert fx["actor_p32_%d" % u].shape == (AG.N_PARAMS,) and fx["critic_p64_%d" % u].shape == (CG.N_PARAMS - 58,)


def test_actor_chain_within_8x_of_the_references_own_fp32():
    fx, hyper = O.fixture(), O.fixture_hyper()
    act, fn, c = O.actor_case()
    clip, coef_ent, R = float(fx["clip_param"]), float(fx["entropy_coef"]), AG.R
    p = O.sd_flat(c["sd"], AG.FIELDS, AG.KEYS, AG.SHAPES)
    m, v, st, results = np.zeros_like(p), np.zeros_like(p), O.new_state(), []
    for u in range(O.UPDATES):
        sd = O.flat_sd(p, c["sd"], AG.FIELDS, AG.KEYS, AG.SHAPES)
        lg = AG.backward(sd, c["obs"], c["actions"], np.zeros(R), 0.0, act)["logits"]
        zc = lg - lg.max(-1, keepdims=True)
        logp = zc - np.log(np.exp(zc).sum(-1, keepdims=True))
        new = np.take_along_axis(logp, c["actions"].astype(np.int64), -1)
        _, r, _, d = AG.dlogp(np.repeat(new, 3, -1), np.repeat(c["old_log_probs"], 3, -1), c["advantages"][:, 0], 0, clip,
                              factor=c["factor"][:, 0], scale=1.0 / R, fp32_inputs=False)
        g = AG.flat(AG.backward(sd, c["obs"], c["actions"], d, -coef_ent / R, act)).astype(np.float32)
        p, m, v, norm = O.step(g, p, m, v, st, first=0 if fn else 52, **hyper)
        assert abs(norm - float(fx["actor_grad_norm32"][u])) <= 1e-4 * norm
        results.append(p)
    d, d32 = O.fixture_distance(results, "actor")
    print("actor chain: %.3e from the reference's fp64 results, the reference's fp32 results %.3e: ratio %.2f" % (d, d32, d / d32))
    assert d32 > 0.0 and d <= MARGIN * d32


def test_critic_chain_within_8x_of_the_references_own_fp32():
    fx, hyper = O.fixture(), O.fixture_hyper()
    act, fn, c = O.critic_case()
    clip, delta, coef, R = float(fx["clip_param"]), float(fx["huber_delta"]), float(fx["value_loss_coef"]), CG.R
    p = O.sd_flat(c["sd"], CG.FIELDS, CG.KEYS, CG.SHAPES)
    m, v, st, results = np.zeros_like(p), np.zeros_like(p), O.new_state(), []
    for u in range(O.UPDATES):
        sd = O.flat_sd(p, c["sd"], CG.FIELDS, CG.KEYS, CG.SHAPES)
        scale, shift = value_norm_scale_shift((fx["critic_norm_mean"][u], fx["critic_norm_var"][u]))
        raw = CG.backward(sd, c["share_obs"], np.zeros(R), act)["u"]
        vl = CG.value_loss(raw, c["value_preds"][:, 0], c["returns"][:, 0], scale, shift, clip, delta, CG.HUBER | CG.CLIPPED, coef / R)
        g = CG.flat(CG.backward(sd, c["share_obs"], (coef / R) * vl["g"], act)).astype(np.float32)
        p, m, v, norm = O.step(g, p, m, v, st, first=0 if fn else 58, **hyper)
        assert abs(norm - float(fx["critic_grad_norm32"][u])) <= 1e-4 * norm
        results.append(p)
    d, d32 = O.fixture_distance(results, "critic")
    print("critic chain: %.3e from the reference's fp64 results, the reference's fp32 results %.3e: ratio %.2f" % (d, d32, d / d32))
    assert d32 > 0.0 and d <= MARGIN * d32
    assert not fn and not np.asarray(results[-1])[:58].any()      # (no feature LayerNorm: its entries stay as set)
