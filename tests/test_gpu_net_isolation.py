"""Stepping one network touches no other: one engine of 64 envs with three actors and the critic set; each of the four in turn takes one
backward over 17 stored rows (one full 16-row tile and one ragged row) and one Adam step with clipping active and weight decay 0.01,
and after each step everything the library keeps for the three OTHER networks has the bits it had before the step --
  their parameters (actor_state_dict / critic_state_dict) and their optim_state (m, v, step, powers, skipped);
  their packed copies, as seen through actor_logits / critic_raw_values on the 17 rows (the evaluate pack), a second backward over the
  17 rows (the transposed pack), and a 2-step rollout_actor with logits after a reset() (the closed-loop pack) --
while the stepped network's own parameters, optimiser state and every one of these views have moved.  This is the mistake a shared
record of "a network" invites (a wrong slot base, a pack pointer of the neighbouring slot) and the twin-engine tests of one slot in
tests/test_gpu_optim.py cannot see.

The closed loop: every rollout starts from the same restored snapshot behind its reset().  Its first step's logits are a function of
the restored observations and one actor alone; its second step's are compared for the envs whose first actions are the ones chosen
before the step (there the envs' states, and so every other actor's inputs, are the same bits)."""
import numpy as np
import pytest

from tests import actor_ref as AR
from tests import critic_ref as CR

pytestmark = pytest.mark.gpu

N, ROWS = 64, 17
NETS = (0, 1, 2, "critic")
ADAM = dict(lr=1e-3, weight_decay=0.01, max_grad_norm=1e-3)


def same(a, b):
    """two views of a network: the same keys, every array the same bits"""
    assert set(a) == set(b)
    return all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


class Rows:
    """the 17 stored rows and the coefficients of the backward calls, on the engine's device"""

    def __init__(self, eng):
        import torch
        rng = np.random.default_rng(91)
        put = lambda x: torch.from_numpy(x).to(eng.device)
        self.obs = put(rng.standard_normal((ROWS, 26)).astype(np.float32))
        self.share = put(rng.standard_normal((ROWS, 29)).astype(np.float32))
        self.actions = put(rng.integers(0, 3, ROWS).astype(np.int32))
        self.coef = [put(rng.standard_normal(ROWS).astype(np.float32)) for _ in range(2)]      # the step's backward, the probe's

    def backward(self, eng, which, i):
        if which == "critic":
            return eng.critic_backward(self.share, self.coef[i])
        return eng.actor_backward(which, self.obs, self.actions, self.coef[i], dent=-0.01 / ROWS, per_agent=False)

    def forward(self, eng, which):
        return eng.critic_raw_values(self.share) if which == "critic" else eng.actor_logits(which, self.obs, per_agent=False)


def view(eng, rows, which):
    """everything the library keeps for one network, but the closed-loop pack: host arrays"""
    sd = eng.critic_state_dict() if which == "critic" else eng.actor_state_dict(which)
    out = {"param." + k: v.numpy().copy() for k, v in sd.items()}
    st = eng.optim_state(which)
    out.update({"optim." + k: np.asarray(st[k]) for k in ("m", "v", "step", "beta1_pow", "beta2_pow", "skipped")})
    out["forward"] = rows.forward(eng, which).cpu().numpy()
    g = rows.backward(eng, which, 1)
    out["backward"], out["backward.sq"] = g.flat.cpu().numpy(), g.sq_norm.cpu().numpy()
    return out


def closed_loop(eng, snap):
    """two steps of the three actors from the snapshot's state -> (actions [2, N, 3], logits [2, N, 3, 3], obs [2, N, 3, 26]) on the host"""
    eng.reset()
    eng.restore(snap)
    out = eng.rollout_actor(2, sample=False, want_logits=True)
    return out[5].cpu().numpy(), out[6].cpu().numpy(), out[0].cpu().numpy()


@pytest.mark.parametrize("activation,feature_norm", [("tanh", True), ("relu", False)])
def test_stepping_one_network_touches_no_other(activation, feature_norm):
    eng = AR.engine(N, False)
    try:
        AR.set_actors(eng, [AR.torch_actor(410 + a, activation, feature_norm=feature_norm) for a in range(3)], activation)
        eng.set_critic(CR.make_critic(420, feature_norm), CR.VALUE_NORM, activation)
        eng.reset()
        snap = eng.snapshot()
        rows = Rows(eng)
        before = {w: view(eng, rows, w) for w in NETS}
        loop = closed_loop(eng, snap)
        assert all(same({"x": x}, {"x": y}) for x, y in zip(loop, closed_loop(eng, snap)))      # (the probe itself repeats to the bit)
        for w in NETS:
            norm = (eng.critic_adam_step if w == "critic" else lambda g, **kw: eng.actor_adam_step(w, g, **kw))(rows.backward(eng, w, 0), **ADAM)
            assert float(norm.cpu()) > ADAM["max_grad_norm"], (w, "the clipping is active")
            after = {o: view(eng, rows, o) for o in NETS}
            for o in NETS:
                if o != w:
                    assert same(before[o], after[o]), (w, o, [k for k in before[o] if not same({k: before[o][k]}, {k: after[o][k]})])
            moved = [k for k in before[w] if not same({k: before[w][k]}, {k: after[w][k]})]
            params = [k for k in before[w] if k.startswith("param.") and (feature_norm or "feature_norm" not in k)]
            assert set(moved) >= set(params) | {"optim.m", "optim.v", "optim.step", "optim.beta1_pow", "optim.beta2_pow", "forward", "backward"}, (w, moved)
            assert int(after[w]["optim.step"]) == int(before[w]["optim.step"]) + 1 and int(after[w]["optim.skipped"]) == 0
            acts, logits, obs = closed_loop(eng, snap)
            if w == "critic":      # (no actor moved: the whole closed loop keeps its bits)
                assert same(dict(a=acts, l=logits, o=obs), dict(a=loop[0], l=loop[1], o=loop[2]))
            else:
                kept = (acts[0] == loop[0][0]).all(axis=-1)      # envs whose first actions are the ones chosen before the step
                assert kept.any(), w      # (else the second step's comparison would be empty)
                assert same({"o": obs[0][kept]}, {"o": loop[2][0][kept]})
                for o in (0, 1, 2):
                    first = same({"l": logits[0, :, o]}, {"l": loop[1][0, :, o]})
                    second = same({"l": logits[1, kept, o]}, {"l": loop[1][1, kept, o]})
                    assert (first, second) == ((True, True) if o != w else (False, False)), (w, o, first, second)
            before, loop = after, (acts, logits, obs)
    finally:
        eng.close()
