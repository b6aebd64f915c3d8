"""The critic and the stored-row actors run ONE network (csrc/sdc_rowmlp.hpp): where the two networks are the same, the values and the
logits are the same bits.

An actor with feature normalisation off, and for each of its three logit columns c a critic with feature normalisation off whose
w1[:, :26] is the actor's and w1[:, 26:] = 0, whose b1, hidden LayerNorms, w2 and b2 are the actor's, w3 = actor.w3[c], b3 = actor.b3[c],
no value norm (scale 1, shift 0).  On share_obs rows X [n, 29] with finite random entries critic_values(X) equals
actor_logits(agent, X[:, :26])[:, c] bit for bit: a zero weight times a finite entry adds +-0 to an accumulator that is not zero (it
starts at b1), the critic's eighth k-step of layer 1 adds zeros only, and the two heads sum the four lane groups in the same pairing.

n in 1, 15, 16, 17, 65: a lone row, a part-filled tile, a full one, one row past it, a second workgroup.  Both activations, one engine of
two envs.  No tolerance: bits."""
import numpy as np
import pytest

from tests import actor_ref as AR

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 15, 16, 17, 65)


@pytest.fixture(scope="module")
def eng():
    e = AR.engine(2, False)
    yield e
    e.close()


def _actor(seed):
    """sdc_actor_params' fields, every one random (torch's Linear bounds, LayerNorm gains about 1), no feature LayerNorm"""
    r = np.random.default_rng(seed)
    u = lambda shape, fan_in: ((r.random(shape) * 2 - 1) / np.sqrt(fan_in)).astype(np.float32)
    p = {"w1": u((64, 26), 26), "b1": u((64,), 26), "w2": u((64, 64), 64), "b2": u((64,), 64), "w3": u((3, 64), 64), "b3": u((3,), 64)}
    for k in ("ln1", "ln2"):
        p[k + "_gamma"] = (1.0 + 0.2 * r.standard_normal(64)).astype(np.float32)
        p[k + "_beta"] = (0.2 * r.standard_normal(64)).astype(np.float32)
    return p


def _critic_of(actor, c):
    w1 = np.zeros((64, 29), np.float32)
    w1[:, :26] = actor["w1"]
    return {"w1": w1, "b1": actor["b1"], "ln1_g": actor["ln1_gamma"], "ln1_b": actor["ln1_beta"], "w2": actor["w2"], "b2": actor["b2"],
            "ln2_g": actor["ln2_gamma"], "ln2_b": actor["ln2_beta"], "w3": actor["w3"][c].copy(), "b3": actor["b3"][c]}


@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_the_critic_and_an_actor_give_the_same_bits_where_the_network_is_the_same(eng, activation):
    import torch
    agent = 1
    actor = _actor(31 + (activation == "relu"))
    eng.set_actor(agent, dict(actor, activation=activation))
    X = torch.randn((max(ROW_COUNTS), 29), generator=torch.Generator().manual_seed(17)).to(eng.device)
    assert bool(X.isfinite().all()) and float(X[:, 26:].abs().min()) > 0.0      # (the columns the critic's zero weights meet are live)
    logits = {n: eng.actor_logits(agent, X[:n, :26].contiguous()) for n in ROW_COUNTS}
    for c in range(3):
        eng.set_critic(_critic_of(actor, c), None, activation)
        for n in ROW_COUNTS:
            v = eng.critic_values(X[:n].contiguous())
            assert v.shape == (n,) and logits[n].shape == (n, 3) and bool(v.isfinite().all())
            same = v.view(torch.int32) == logits[n][:, c].contiguous().view(torch.int32)
            assert bool(same.all()), (activation, c, n, int((~same).sum()), float((v - logits[n][:, c]).abs().max()))
        assert float(logits[65][:, c].std()) > 1e-3      # (the column is a function of the rows, not a constant)
