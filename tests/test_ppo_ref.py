"""tests/ppo_ref.py -- the NumPy restatement of sdc_ppo_terms the GPU tests hold the kernels to -- held, without a GPU, to what the
REFERENCE returned: tests/golden/actor_eval/actor_eval.npz stores, for four networks, the inputs and outputs of the reference's
StochasticPolicy.evaluate_actions and HAPPO.update over 67 rows (tests/golden/gen_actor_eval_golden.py).

THE BOUND is derived from the reference's own fp32 chain, not from the observed difference.  The restatement starts from the fixture's
fp32 logits (tests/onpolicy_ref.action_log_probs: fp64, rounded once to fp32) and works in fp64; the reference works in fp32.  With
u = 2^-24 (half an ulp, relative), every fp32 operation of the reference contributing u times its result, and z_i = l_i - max l:
  log_softmax   z_i: u |z_i|;  e_i = exp z_i: its input's error times e_i, and u e_i;  s = e0 + e1 + e2 <= 3: the largest relative
                error of its terms, (zmax + 1) u, and two additions, 2 u;  log s: s's relative error, and u |log s| <= u log 3;
                lp_j = z_j - log s: u |z_j| + (zmax + 3 + log 3) u + u |lp_j|          =: E_ref
                the restatement's own log-probability is rounded once: u |lp_j|         =: E_own
  new - old     the reference's fp32 subtraction: u |d|;  the restatement's is exact:  E_d = E_ref + E_own + u |d|
  exp           its input's error times the ratio, and u r:                              E_r = r (E_d + u)          (the reference's r)
  imp_weights   both are fp32 values; the restatement's ratio is rounded once more:      |imp - ratio| <= E_r + u r
  products      s1 = r A: |A| E_r + u |s1|;  the clamp's bounds 1 -+ clip are fp32 in the reference, u 1.2 off, so the clamped
                ratio is off by max(E_r, 1.2 u);  s2: |A| max(E_r, 1.2 u) + u |s2|
  min           at most the larger of the two:                                            E_m = |A| max(E_r, 1.2 u) + u max(|s1|, |s2|)
  factor * min  F E_m + u |F m| for the reference's product, u |F m| for the restatement's one rounding of surr
  the mean      the mean of the terms' errors, and at most 2^-24 of the mean absolute term for the reference's fp32 summation
each first-order bound widened by SLACK = 1.01 for the products of errors left out.  The fp64 arithmetic of the restatement itself
(2^-53 relative per operation) is three thousand million times smaller and is left out.

Observed on the fixture (printed by the tests): imp_weights at most 4.8e-7 from the restatement's ratio, 0.30 to
0.38 of the row's own bound; policy_loss 4.7e-9 to 2.1e-8 off against bounds of 7.2e-7 to 7.9e-7."""
import numpy as np
import pytest

from tests import actor_eval_ref as AE
from tests import onpolicy_ref as OR
from tests import ppo_ref as PR

U = 2.0 ** -24
SLACK = 1.01


def _chain(c, agent):
    """the restatement on one configuration's rows, laid out as T = 67 steps of one env with the agent's column live and the other
    two NaN; -> (terms, stats, the per-row bounds of imp_weights, the bound of policy_loss)"""
    n = AE.R
    logits3 = np.full((n, 1, 3, 3), np.nan, dtype=np.float32)
    logits3[:, 0, agent] = c["logits"]
    acts3 = np.zeros((n, 1, 3), dtype=np.int32)
    acts3[:, 0, agent] = c["actions"][:, 0]
    with np.errstate(invalid="ignore"):
        new, ent = OR.action_log_probs(acts3, logits3)
    old = np.full((n, 1, 3), np.nan, dtype=np.float32)
    old[:, 0, agent] = c["old_log_probs"][:, 0]
    t = PR.terms(new, old, c["advantages"], agent, float(AE.fixture()["clip_param"]), c["factor"])
    s = PR.stats(t["surr"], t["ratio"], t["lr"], ent[..., agent], t["clipped"])
    # the bound, row by row
    l = c["logits"].astype(np.float64)
    z = l - l.max(-1, keepdims=True)
    zmax = np.abs(z).max(-1)
    lp = new[:, 0, agent].astype(np.float64)
    zj = np.take_along_axis(z, c["actions"].astype(np.int64), -1)[:, 0]
    e_ref = U * (np.abs(zj) + zmax + 3.0 + np.log(3.0) + np.abs(lp))
    e_d = e_ref + U * np.abs(lp) + U * np.abs(t["lr"][:, 0])
    r = t["r"][:, 0]
    e_r = SLACK * r * (e_d + U)
    A, F = np.abs(c["advantages"][:, 0].astype(np.float64)), c["factor"][:, 0].astype(np.float64)
    lo, hi = 1.0 - float(AE.fixture()["clip_param"]), 1.0 + float(AE.fixture()["clip_param"])
    s1, s2 = r * A, np.clip(r, lo, hi) * A
    e_m = A * np.maximum(e_r, 1.2 * U) + U * np.maximum(s1, s2)
    fm = np.abs(t["surr"][:, 0].astype(np.float64))
    e_term = SLACK * (F * e_m + 2.0 * U * fm)
    return t, s, e_r + U * r, float(e_term.mean() + U * fm.mean())


@pytest.mark.parametrize("activation,feature_norm", AE.CONFIGS)
@pytest.mark.parametrize("agent", [0, 1, 2])
def test_restatement_gives_the_references_imp_weights_and_policy_loss(activation, feature_norm, agent):
    c = AE.case(activation, feature_norm)
    t, s, bound_r, bound_loss = _chain(c, agent)
    d_r = np.abs(t["ratio"][:, 0].astype(np.float64) - c["imp_weights"][:, 0].astype(np.float64))
    loss = PR.summary(s)["policy_loss"]
    d_loss = abs(loss - float(c["policy_loss"]))
    print("%s agent %d: imp_weights max |difference| %.2e (largest share of its bound %.2f); policy_loss %.7f against %.7f: %.2e "
          "(bound %.2e)" % (AE.cfg_name(activation, feature_norm), agent, d_r.max(), (d_r / bound_r).max(), loss,
                            float(c["policy_loss"]), d_loss, bound_loss))
    assert (d_r <= bound_r).all(), (d_r / bound_r).max()
    assert d_loss <= bound_loss, (d_loss, bound_loss)
    # some rows of the fixture have a ratio of exactly one (in the reference: its own log-probabilities were the old ones), some an
    # advantage of exactly zero, and the clip is live on both sides
    assert (c["imp_weights"] == 1.0).sum() >= 5 and (c["advantages"] == 0).sum() >= 4
    assert (t["r"] < 0.8).any() and (t["r"] > 1.2).any() and not t["unsure"].any()


def test_ordered_sums_follow_the_two_stage_order():
    """`ordered` against the order written out element by element, at sizes on both sides of one workgroup, of the stage-1 cap and of
    stage 2's loop"""
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 700, 256 * 300 + 5, 256 * PR.MAX_BLOCKS + 77):
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
        B = PR.blocks(n)
        assert B == min(-(-n // 256), 1024)
        lane = [[0.0] * 256 for _ in range(B)]
        for i in range(n):
            b, l = (i // 256) % B, i % 256
            lane[b][l] = lane[b][l] + x[i]

        def halve(v):
            v = list(v)
            half = 128
            while half >= 1:
                for l in range(half):
                    v[l] = v[l] + v[l + half]
                half //= 2
            return v[0]

        part = [halve(v) for v in lane]
        acc = [0.0] * 256
        for b in range(B):
            acc[b % 256] = acc[b % 256] + part[b]
        want = halve(acc)
        assert PR.ordered(x, "sum") == want, n
        assert PR.ordered(x, "min") == x.min() and PR.ordered(x, "max") == x.max()
    assert PR.blocks(256 * 1024) == 1024 and PR.blocks(256 * 1024 + 1) == 1024 and PR.blocks(256 * 1023 + 1) == 1024


def test_terms_at_the_edges():
    """a ratio of exactly one, lr of +-80 (finite in fp32), clip_param 0 (everything but r = 1 is clipped), zero advantages, no factor"""
    new = np.zeros((6, 1, 3), dtype=np.float32)
    old = np.zeros((6, 1, 3), dtype=np.float32)
    new[:, 0, 1] = [0.0, 80.0, -80.0, 0.25, -0.25, 0.0]
    adv = np.array([[1.0], [2.0], [-1.0], [0.0], [-3.0], [-2.0]], dtype=np.float32)
    t = PR.terms(new, old, adv, 1, 0.0)
    assert t["ratio"][0, 0] == 1.0 and np.isfinite(t["ratio"]).all() and t["ratio"][2, 0] > 0
    assert list(t["clipped"][:, 0]) == [False, True, True, True, True, False]
    # clip 0: the clamped ratio is 1, so surr = min(r A, A)
    want = np.minimum(t["r"][:, 0] * adv[:, 0].astype(np.float64), adv[:, 0].astype(np.float64)).astype(np.float32)
    assert np.array_equal(t["surr"][:, 0], want)
    assert np.array_equal(t["factor_out"], t["ratio"])
    s = PR.summary(PR.stats(t["surr"], t["ratio"], t["lr"], None, t["clipped"]))
    assert s["entropy"] == 0.0 and s["clip_frac"] == 4 / 6 and s["approx_kl"] == 0.0 and s["ratio_max"] == float(t["ratio"][1, 0])
