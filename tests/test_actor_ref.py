"""tests/actor_ref.py -- the host restatement tests/test_gpu_actor_head.py holds the device's policy head to -- checked on its own,
without a GPU: the reference must be right before anything is compared with it, and the unsure share of the constant-logit launches,
which follows from Philox alone, must meet the cap for the seed the GPU test uses (another seed is chosen here if it does not)."""
import numpy as np
import pytest

from tests import actor_ref as R
from tests.reset_ref import philox4x32_10


def test_uniforms_are_the_stated_words_of_the_stated_block():
    ep = np.array([1, 2, 1, 7])
    u = R.uniforms(R.HIGH_SEED, R.BASE, ep, [0, 5, 95])
    assert u.shape == (3, 4, 3) and u.min() >= 0.0 and u.max() < 1.0
    assert (u * 2.0 ** 24 == np.floor(u * 2.0 ** 24)).all()
    # one block spelled out: step 5, env 2 (global BASE + 2), episode 1
    x, y, z, _ = philox4x32_10(5, R.BASE + 2, 1, 0xAC70, 7, 0x9E3779B9)
    assert [u[1, 2, a] for a in range(3)] == [(int(w) >> 8) / 16777216.0 for w in (x, y, z)]
    # every key component is live
    for other in (R.uniforms(R.HIGH_SEED & 0xFFFFFFFF, R.BASE, ep, [0, 5, 95]), R.uniforms(R.HIGH_SEED, 0, ep, [0, 5, 95]),
                  R.uniforms(R.HIGH_SEED, R.BASE, ep + 1, [0, 5, 95]), R.uniforms(R.HIGH_SEED, R.BASE, ep, [1, 6, 96])):
        assert (other != u).mean() > 0.9


def test_draw_ref_is_the_inverse_cdf_of_the_softmax():
    l = np.float32([0.3, -1.2, 0.9])
    p = np.exp(l.astype(np.float64))
    p /= p.sum()
    eps = 1e-4
    for u, want in ((0.0, 0), (p[0] - eps, 0), (p[0] + eps, 1), (p[0] + p[1] - eps, 1), (p[0] + p[1] + eps, 2), (1.0 - 2.0 ** -24, 2)):
        a, unsure = R.draw_ref(l, u)
        assert a == want and not unsure, (u, a, unsure)
    assert R.draw_ref(l, p[0] + 0.5e-5)[1] and R.draw_ref(l, p[0] + p[1] - 0.5e-5)[1]      # inside the band
    # the band's share on the 24-bit grid: two thresholds, 2 BAND wide each
    u = np.arange(0, 2 ** 24, 7, dtype=np.float64) * 2.0 ** -24
    a, unsure = R.draw_ref(np.broadcast_to(l, (len(u), 3)), u)
    assert abs(unsure.mean() - 4 * R.BAND) < 2e-6
    np.testing.assert_allclose(np.bincount(a, minlength=3) / len(u), p, atol=1e-6)
    # the degenerate cases as the GPU test states them (fp64 keeps e = 2^-288 where fp32 has 0: u = 0 is the one case that differs,
    # which is why the GPU test asserts these outright and not through the band)
    for b3, c in R.ALWAYS.items():
        a, _ = R.draw_ref(np.broadcast_to(np.float32(b3), (len(u), 3)), u)
        assert (a[1:] == c).all()
    a, _ = R.draw_ref(np.broadcast_to(np.float32(R.HALVES), (len(u), 3)), u)
    np.testing.assert_array_equal(a, np.where(u < 0.5, 0, 2))


def test_the_tie_patterns_are_all_thirteen_at_distinct_fp32_levels():
    pats = R.order_patterns()
    assert len(set(pats)) == 13 and (0, 0, 0) in pats and (1, 1, 0) in pats and (2, 1, 0) in pats
    for lv in R.TIE_LEVELS:
        assert lv.dtype == np.float32 and lv[0] < lv[1] < lv[2]
    assert len(R.tie_b3()) == 26
    # first maximum
    for p, first in (((0, 0, 0), 0), ((1, 1, 0), 0), ((0, 1, 1), 1), ((1, 0, 1), 0), ((0, 1, 0), 1), ((0, 0, 1), 2), ((1, 2, 2), 1)):
        assert R.mode_ref(np.float32(p)) == first


@pytest.mark.parametrize("N", [n for n, _ in R.SHAPES])
def test_constant_logit_launches_meet_the_unsure_cap_by_the_rule_alone(N):
    share = R.constant_unsure_share(N)
    print("constant-logit launches, N = %d, seed %d: unsure share %.2e" % (N, R.CONSTANT_SEED, share))
    assert share <= R.UNSURE_CAP
