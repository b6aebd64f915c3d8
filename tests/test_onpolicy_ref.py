"""The NumPy restatement of the on-policy batch (tests/onpolicy_ref.py) against the reference itself, without a GPU: its returns equal
those of the reference's OnPolicyCriticBufferEP.compute_returns bit for bit on tests/golden/onpolicy/onpolicy_returns.npz (T = 37, N = 65; three
(gamma, gae_lambda) pairs x use_gae on / off; done flags at the first step, the last step, on consecutive steps and nowhere; one case
through a real ValueNorm), and its moments equal np.nanmean / np.nanstd taken in fp64 to 1e-12 relative.  The fixture is written by
tests/golden/gen_onpolicy_golden.py, which imports the reference and copies none of it."""
import os

import numpy as np
import pytest

from tests import onpolicy_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "onpolicy", "onpolicy_returns.npz")
REL = 1e-12


@pytest.fixture(scope="module")
def fx():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rew3(fx):
    """the fixture's rewards as column 0 of a [T, N, 3] array whose other columns must not be read"""
    r = np.full(fx["rew"].shape + (3,), np.nan, dtype=np.float32)
    r[..., 0] = fx["rew"]
    return r


def test_fixture_holds_what_it_says(fx):
    T, N = fx["done"].shape
    assert (T, N) == (37, 65) and fx["values"].shape == (38, 65) and fx["rew"].dtype == np.float32 and fx["done"].dtype == np.uint8
    assert [tuple(x) for x in fx["gamma_lambda"]] == list(R.GAMMA_LAMBDA)
    d = fx["done"]
    assert d[0].any() and d[T - 1].any() and (d[:-1] & d[1:]).any() and (d.sum(0) == 0).any()
    assert os.path.getsize(FIXTURE) < 200 * 1024


def test_returns_are_the_references_bit_for_bit(fx):
    for i, (gamma, lam) in enumerate(R.GAMMA_LAMBDA):
        for use_gae in (0, 1):
            ret, adv, masks = R.gae(_rew3(fx), fx["done"], fx["values"], gamma, lam, bool(use_gae))
            want = fx[f"plain_returns_{i}_{use_gae}"]
            assert np.array_equal(_bits(ret), _bits(want)), (gamma, lam, use_gae, int((_bits(ret) != _bits(want)).sum()))
            assert np.array_equal(_bits(adv), _bits(want - fx["values"][:-1]))
            assert np.array_equal(masks[1:], 1.0 - fx["done"]) and (masks[0] == 1.0).all()
    # (the cases differ: a restatement that ignored gamma, lambda or use_gae would not pass them all)
    assert len({fx[k].tobytes() for k in fx if k.startswith("plain_returns_")}) == 6


def test_returns_through_a_real_value_norm(fx):
    """the reference denormalises the raw predictions itself; the restatement is fed ValueNorm.denormalize of them"""
    gamma, lam = R.GAMMA_LAMBDA[0]
    ret, _, _ = R.gae(_rew3(fx), fx["done"], fx["norm_values"], gamma, lam, True)
    assert np.array_equal(_bits(ret), _bits(fx["norm_returns"]))
    # the value predictions the kernel recomputes from the denormalised values come back to the raw ones within a few ulp of the values
    deb = max(float(fx["norm_debiasing_term"]), 1e-5)
    mean = np.float32(fx["norm_running_mean"][0]) / np.float32(deb)
    var = max(np.float32(fx["norm_running_mean_sq"][0]) / np.float32(deb) - mean * mean, np.float32(1e-2))
    back = R.value_preds(fx["norm_values"], np.sqrt(np.float32(var)), mean)
    err = np.abs(back.astype(np.float64) - fx["norm_raw"]).max()
    tol = 4 * np.spacing(np.abs(fx["norm_values"]).max()) / float(np.sqrt(var))
    print("value_preds against the raw predictions: max |difference| %.3e (bound %.3e)" % (err, tol))
    assert err <= tol


def test_first_done_and_reward_agent():
    rew, values = R.inputs(5, 7, 3)
    done = R.done_pattern("staggered", 5, 7)
    first = (np.arange(7) % 3 == 0).astype(np.uint8)
    base = R.gae(rew, done, values, 0.99, 0.95)
    ret, adv, masks = R.gae(rew, done, values, 0.99, 0.95, first_done=first)
    assert np.array_equal(masks[0], 1.0 - first) and np.array_equal(masks[1:], base[2][1:]) and np.array_equal(_bits(ret), _bits(base[0]))
    other = R.gae(rew, done, values, 0.99, 0.95, reward_agent=2)
    swapped = R.gae(rew[..., ::-1].copy(), done, values, 0.99, 0.95, reward_agent=0)
    assert np.array_equal(_bits(other[0]), _bits(swapped[0])) and not np.array_equal(_bits(other[0]), _bits(base[0]))


@pytest.mark.parametrize("magnitude", [1e-3, 1.0, 1e3])
def test_moments_are_nanmean_and_nanstd(fx, magnitude):
    worst = 0.0
    cases = [R.gae(_rew3(fx), fx["done"], fx["values"] * np.float32(magnitude), g, l, bool(u))[1]
             for g, l in R.GAMMA_LAMBDA for u in (0, 1)]
    cases.append(R.gae(*_inputs_300(magnitude), 0.99, 0.95)[1])      # more envs than the tree has leaves
    for adv in cases:
        mean, std = R.moments(adv)
        a = adv.astype(np.float64)
        want = (float(np.nanmean(a)), float(np.nanstd(a)))
        worst = max(worst, abs(mean - want[0]) / abs(want[0]), abs(std - want[1]) / want[1])
    print("moments against np.nanmean / np.nanstd at magnitude %g: max relative difference %.2e" % (magnitude, worst))
    assert worst <= REL


def _inputs_300(magnitude):
    rew, values = R.inputs(9, 300, 11, magnitude)
    return rew, R.done_pattern("staggered", 9, 300), values


def test_log_probs_are_log_softmax():
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((11, 13, 3, 3)) * 2.5).astype(np.float32)
    logits[0, 0, 0] = (0.0, 80.0, -80.0)      # probabilities that underflow in fp32, not in fp64
    actions = rng.integers(0, 3, (11, 13, 3))
    actions[0, 0, 0] = 2
    lp, ent = R.action_log_probs(actions, logits)
    assert lp.dtype == ent.dtype == np.float32 and lp.shape == ent.shape == (11, 13, 3)
    l = logits.astype(np.float64)
    want = l - np.log(np.exp(l - l.max(-1, keepdims=True)).sum(-1, keepdims=True)) - l.max(-1, keepdims=True)
    wj = np.take_along_axis(want, actions[..., None], -1)[..., 0]
    assert np.abs(lp - wj).max() <= 1e-6 * np.abs(wj).max() and lp[0, 0, 0] == np.float32(-160.0)
    p = np.exp(want)
    assert np.abs(ent + (p * want).sum(-1)).max() <= 1e-6 and (ent >= 0).all() and ent.max() <= np.float32(np.log(3.0)) + 1e-6
    # how often fp64 itself, against extended precision, moves the rounded result: the share the GPU test's bar leaves room for
    lp80, ent80 = R.action_log_probs(actions, logits, np.longdouble)
    share = float((R.ulps(lp, lp80) > 0).mean()), float((R.ulps(ent, ent80) > 0).mean())
    print("fp64 against long double after the rounding to fp32: share of results that differ %.2e (log-prob), %.2e (entropy)" % share)
    assert R.ulps(lp, lp80).max() <= 1 and R.ulps(ent, ent80).max() <= 1
