"""The NumPy restatement of TRAIN ON THE DEVICE (tests/train_ref.py) held to what it restates, without a GPU: the permutation is a
bijection at every size the code takes another path at, keyed on seed and stream, and over 4096 streams its position-by-value counts
pass a chi-square test (the bars are the test's: e = 4096 / n per cell, a cell within 6 sd, the statistic at most dof + 4 sqrt(2 dof));
ValueNorm's update equals the reference's own fp32 ValueNorm (the fixture tests/golden/train/train.npz) bit for bit and lies next to a
torch fp64 run of the same recurrence."""
import os

import numpy as np
import pytest

from tests import train_ref as TR

SIZES = [1, 2, 3, 5, 17, 800, 1025, 4097, 672 * 4096]


@pytest.mark.parametrize("n", SIZES)
def test_permutation_is_a_bijection(n):
    p, passes = TR.permutation(n, seed=20260101, stream_id=(2 << 32) | 3)
    assert p.dtype == np.int32 and p.shape == (n,)
    seen = np.zeros(n, dtype=bool)
    seen[p] = True
    assert seen.all() and p.min() == 0 and p.max() == n - 1
    assert 4 ** TR.half_bits(n) >= n and (n < 2 or 4 ** TR.half_bits(n) < 4 * n)
    print("n", n, "b", TR.half_bits(n), "passes of the slowest index", passes)


def test_seed_and_stream_key_the_permutation():
    n = 800
    base = TR.permutation(n, 7, 0)[0]
    assert np.array_equal(base, TR.permutation(n, 7, 0)[0])
    others = [TR.permutation(n, 8, 0)[0], TR.permutation(n, 7 | (1 << 40), 0)[0], TR.permutation(n, 7, 1)[0], TR.permutation(n, 7, 1 << 32)[0]]
    for i, p in enumerate(others):
        assert (p != base).mean() > 0.9, i      # (a random pair agrees in 1 / n of the positions)
    assert len({p.tobytes() for p in others + [base]}) == 5
    assert np.array_equal(TR.permutations(n, 7, [0, 1])[0][1], others[2])


@pytest.mark.parametrize("n", [3, 5, 12, 16, 40])
def test_position_by_value_counts_look_uniform(n):
    S = 4096
    cnt = TR.position_value_counts(n, 99, S)
    assert (cnt.sum(0) == S).all() and (cnt.sum(1) == S).all()
    e = S / n
    sd = np.sqrt(e * (1 - 1 / n))
    chi2, dof = float(((cnt - e) ** 2 / e).sum()), (n - 1) ** 2
    bar = dof + 4 * np.sqrt(2 * dof)
    print("n", n, "chi-square %.1f on %d degrees of freedom, bar %.1f; worst cell %.2f sd" % (chi2, dof, bar, np.abs(cnt - e).max() / sd))
    assert np.abs(cnt - e).max() <= 6 * sd
    assert chi2 <= bar


def test_four_rounds_fail_the_same_test():
    """why the network has six rounds: at n = 12 four rounds miss the bar that six pass"""
    n, S = 12, 4096
    cnt = TR.position_value_counts(n, 99, S, rounds=4)
    e, dof = S / n, (n - 1) ** 2
    assert float(((cnt - e) ** 2 / e).sum()) > dof + 4 * np.sqrt(2 * dof)


def test_two_stage_sums_are_the_plain_sums_in_another_order():
    rng = np.random.default_rng(3)
    for n in (1, 63, 800, 262144 + 77):
        x = rng.normal(-3.0, 2.0, n).astype(np.float32)
        S1, S2 = TR.two_stage_sums(x)
        assert abs(S1 - float(x.astype(np.float64).sum())) <= 1e-12 * n * 10
        assert abs(S2 - float((x * x).astype(np.float64).sum())) <= 1e-12 * n * 100
    # integers sum exactly in any order: the lane mapping loses and doubles nothing
    x = np.arange(1, 262144 + 78, dtype=np.float32) % 7
    assert TR.two_stage_sums(x) == (float(x.sum(dtype=np.float64)), float((x * x).sum(dtype=np.float64)))


def test_value_norm_update_next_to_torch_fp64():
    """the recurrence in torch fp64 is the truth; the restatement's (scale, shift) may lie as far from it as fp32 rounding of the
    three running values puts them: each is one rounding of a convex combination per update, so after k updates at most k half-ulps
    relative, and scale and shift are quotients of them: 4 k * 2^-24 with room for the square root and the subtraction"""
    import torch
    rng = np.random.default_rng(0)
    st = (np.float32(0), np.float32(0), np.float32(0))
    rm = rsq = deb = torch.zeros((), dtype=torch.float64)
    beta, K = 0.99999, 40
    for u in range(K):
        x = (rng.normal(-3.0, 2.0, 800) * (1 + 0.1 * u)).astype(np.float32)
        st, (scale, shift) = TR.value_norm_update(st, x, beta)
        xd = torch.from_numpy(x).double()
        rm = rm * beta + xd.mean() * (1.0 - beta)
        rsq = rsq * beta + (xd ** 2).mean() * (1.0 - beta)
        deb = deb * beta + (1.0 - beta)
        mean, var = rm / deb.clamp(min=1e-5), (rsq / deb.clamp(min=1e-5) - (rm / deb.clamp(min=1e-5)) ** 2).clamp(min=1e-2)
        d = max(abs(float(scale) - float(var.sqrt())) / float(var.sqrt()), abs(float(shift) - float(mean)) / abs(float(mean)))
        assert d <= 4 * (u + 1) * 2.0 ** -24, (u, d)
    print("after %d updates (scale, shift) lie %.2e (relative) from torch fp64" % (K, d))


def test_fixture_is_data_only_and_small():
    fx = TR.fixture()
    assert os.path.getsize(TR.FIXTURE) <= os.path.getsize(os.path.join(os.path.dirname(TR.FIXTURE), "..", "optim", "optim.npz"))
    assert all(v.dtype.kind in "fi" for v in fx.values()), {k: v.dtype for k, v in fx.items()}
    T, N, E, M = (int(fx[k]) for k in ("T", "N", "epochs", "num_mini_batch"))
    assert (T, N, E, M) == (10, 40, 2, 2)
    for who in ("actor", "critic"):
        perms = fx[who + "_perms"]
        assert perms.shape == (E, T * N) and perms.dtype == np.int32 and all(np.array_equal(np.sort(p), np.arange(T * N)) for p in perms)
    assert fx["actor_p32"].dtype == np.float32 and fx["actor_p64"].dtype == np.float64 and fx["actor_p64"].shape == (6391,)
    assert fx["critic_p32"].shape == (6459,) and fx["value_norm32"].shape == fx["value_norm64"].shape == (E * M, 3)


def test_value_norm_update_against_the_references_own_valuenorm():
    """the reference's ValueNorm inside its VCritic.train, over the mini-batches its generator drew: the restatement's (scale, shift)
    after every update may lie 8 x as far from the reference's fp64 run as the reference's own fp32 run does (the fixture's distance)"""
    fx = TR.fixture()
    returns, idx = fx["returns"].reshape(-1), fx["critic_perms"]
    rows = returns.size // int(fx["num_mini_batch"])
    st, u, d, d32, same = (np.float32(0), np.float32(0), np.float32(0)), 0, 0.0, 0.0, 0
    for e in range(idx.shape[0]):
        for k in range(0, returns.size, rows):
            st, mine = TR.value_norm_update(st, returns[idx[e, k:k + rows]], float(fx["beta"]))
            d = max(d, TR.scale_shift_distance(mine, fx["value_norm64"][u]))
            d32 = max(d32, TR.scale_shift_distance(TR.derive(*fx["value_norm32"][u]), fx["value_norm64"][u]))
            same += int(np.array_equal(np.array(st, dtype=np.float32).view(np.uint32), fx["value_norm32"][u].view(np.uint32)))
            u += 1
    assert u == fx["value_norm32"].shape[0]
    print("ValueNorm restatement: (scale, shift) %.3e from the reference's fp64 run, the reference's fp32 run %.3e: ratio %.2f; "
          "%d of %d updates equal the reference's fp32 values bit for bit" % (d, d32, d / d32, same, u))
    assert d32 > 0.0 and d <= 8.0 * d32
