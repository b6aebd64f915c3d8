"""The critic's and the actors' gradient kernels run ONE backward (csrc/sdc_rowmlp_grad.hpp): where the two networks are the same, the
gradients of the members they share are the same bits.  The backward's counterpart of tests/test_gpu_rowmlp.py.

The networks.  An actor with feature normalisation off, w3[1] = w3[2] = 0 and b3 = 0, every other weight seeded and non-zero; the critic
built from it as tests/test_gpu_rowmlp.py builds its own: w1[:, :26] the actor's and zeros behind, b1, the hidden LayerNorms, w2 and b2
the actor's, w3 = actor.w3[0], b3 = 0, no value norm (scale 1, shift 0).  The critic's rows are the actor's rows padded to 29 with zeros.

The coefficients.  actor_backward with dent = 0 over ONE row gives grads[b3][0] = that row's logit gradient dl_0 exactly (the other
fifteen columns and three wavefronts add zeros, the one fp64 partial is rounded back to the fp32 it was).  Those values are the critic's
dvalue over the same rows: dy2 = (0 + dl_0 w3_0) + dl_1 * 0 + dl_2 * 0 in the actors' head is w3 c in the critic's, to the bit, and from
there on the two instantiations run the same operations on the same values in the same order.

Equal as bits: w2, b2, ln1's gain and bias, b1, and the actor's w1 against the critic's w1[:, :26]; the critic's w1[:, 26:] is the
product with the zero padding: exact zeros.  NOT compared: ln2's gain and bias and w3 -- the critic forms them at the end as products of
its one per-lane sum S, the actors sum them per row (ln2's gain), as a matrix product (w3) and from db3 (ln2's bias): other roundings by
design --, b3 (three logit sums against one), and ln0 (the feature LayerNorm is off: zeros on both sides).

n in 1, 16, 17, 65: a lone lane column, a full tile, a second wavefront with one row, a second workgroup.  Both activations, one engine
of two envs, 65 single-row calls per activation shared by the four row counts.  No tolerance: bits."""
import numpy as np
import pytest

from tests import actor_ref as AR
from tests.test_gpu_rowmlp import _actor, _critic_of

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 16, 17, 65)
AGENT = 1
SAME = (("w2", "w2"), ("b2", "b2"), ("ln1_gamma", "ln1_g"), ("ln1_beta", "ln1_b"), ("b1", "b1"))


@pytest.fixture(scope="module")
def eng():
    e = AR.engine(2, False)
    yield e
    e.close()


@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_the_two_backwards_give_the_same_bits_where_the_network_is_the_same(eng, activation):
    import torch
    actor = _actor(41 + (activation == "relu"))
    actor["w3"][1:] = 0.0
    actor["b3"][:] = 0.0
    assert all(bool((v != 0).all()) for k, v in actor.items() if k not in ("w3", "b3")) and bool((actor["w3"][0] != 0).all())
    eng.set_actor(AGENT, dict(actor, activation=activation))
    eng.set_critic(_critic_of(actor, 0), None, activation)
    n_max = max(ROW_COUNTS)
    g = torch.Generator().manual_seed(23)
    X = torch.randn((n_max, 26), generator=g).to(eng.device)
    share = torch.zeros((n_max, 29), device=eng.device)
    share[:, :26] = X
    actions = torch.randint(0, 3, (n_max,), generator=g, dtype=torch.int32).to(eng.device)
    dlogp = torch.randn((n_max,), generator=g).to(eng.device)
    # each row's dl_0: the actors' kernel over that row alone
    dl0 = torch.stack([eng.actor_backward(AGENT, X[r:r + 1], actions[r:r + 1], dlogp[r:r + 1], 0.0).named()["b3"][0] for r in range(n_max)])
    assert bool(dl0.isfinite().all()) and bool((dl0 != 0).all()) and float(dl0.std()) > 1e-3
    bits = lambda t: t.contiguous().view(torch.int32)
    for n in ROW_COUNTS:
        mine = eng.actor_backward(AGENT, X[:n].contiguous(), actions[:n].contiguous(), dlogp[:n].contiguous(), 0.0).named()
        theirs = eng.critic_backward(share[:n].contiguous(), dl0[:n].contiguous()).named()
        for a, c in SAME:
            same = bits(mine[a]) == bits(theirs[c])
            assert bool(same.all()), (activation, n, a, int((~same).sum()), float((mine[a] - theirs[c]).abs().max()))
            assert float(mine[a].abs().max()) > 0.0, (activation, n, a)      # (a gradient, not zeros on both sides)
        same = bits(mine["w1"]) == bits(theirs["w1"][:, :26])
        assert bool(same.all()), (activation, n, "w1", int((~same).sum()), float((mine["w1"] - theirs["w1"][:, :26]).abs().max()))
        assert float(mine["w1"].abs().max()) > 0.0 and bool((theirs["w1"][:, 26:] == 0).all()), (activation, n)
