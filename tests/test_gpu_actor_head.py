"""The closed loop's POLICY HEAD -- the code between an env's three logits and the action that reaches its env step
(sdc_act::pick_action and the Philox block both actor kernels key it with) -- held to the rule include/sustaindc_hip.h states at
sdc_rollout_actor, and two configurations of the network sdc_set_actor accepts that nothing else runs.

  a. the mode: the action is the FIRST maximum of the device's own fp32 logits (np.argmax), every env, step and agent, no case
     excluded -- random networks, and constant-logit networks (w3 = 0: logits = b3 bit for bit) walking the 13 weak orderings of
     three values, far apart and one fp32 ulp apart;
  b. the draws: u from Philox per (episode step, global env index, episode number; agent = word) on the host, the action from the
     returned logits in fp64 (tests/actor_ref.draw_ref); every case further than 1e-5 of the sum from a threshold must equal the
     device's action, and at most 1e-3 of the cases may be nearer (expected 4e-5; for the constant-logit cases the share follows from
     Philox alone and tests/test_actor_ref.py holds it on the CPU).  A whole episode and the next one's first steps, env_index_base,
     a seed above 2^32, set_seed, episode numbers that differ inside a wavefront, degenerate and skewed distributions;
  c. the network without the feature LayerNorm (a state_dict without base.feature_norm.*), and with a hidden layer whose activations
     are all equal (variance 0 in the LayerNorm), against an fp64 PyTorch restatement on the observations the kernel saw.

Each at N = 40 on the two-envs-per-wavefront kernel (two full workgroups and a part-filled one) and N = 44 on the four-envs one.
Network accuracy with the usual configuration stays with tests/test_gpu_actor.py."""
import numpy as np
import pytest

from tests import actor_ref as R

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize("N,quad", R.SHAPES)


def _mode_holds(launch):
    np.testing.assert_array_equal(launch.actions, R.mode_ref(launch.logits))


# ---------------------------------------------------------------------------------------------------------------- a. the mode
@SHAPES
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_mode_is_the_first_maximum_of_the_returned_logits(N, quad, activation):
    eng = R.engine(N, quad)
    R.set_actors(eng, [R.torch_actor(500 + a, activation) for a in range(3)], activation)
    eng.reset()
    assert (eng.get_state("episode") == 1).all()
    for k in (40, 40, 16):                    # the whole episode
        _mode_holds(R.Launch(eng, k, False, quad))
    assert (eng.get_state("episode") == 2).all()
    eng.close()


@SHAPES
def test_mode_breaks_every_tie_towards_the_first(N, quad):
    """w3 = 0: the logits are b3, bit for bit, whatever the observations; b3 walks the 13 weak orderings of three values at levels
    (0, 1, 2) and at three consecutive fp32 values, three patterns (one per agent) per launch of two steps."""
    eng = R.engine(N, quad)
    b3s = R.tie_b3()
    expect = {(0, 0, 0): 0, (1, 1, 0): 0, (0, 1, 1): 1, (1, 0, 1): 0, (0, 1, 0): 1, (0, 0, 1): 2, (1, 0, 0): 0}
    for p, first in expect.items():           # (the rule itself, spelled out once: np.argmax is the first maximum)
        assert R.mode_ref(np.float32(p)) == first
    b3s += [b3s[0]] * (-len(b3s) % 3)
    seen = set()
    started = False
    for i in range(0, len(b3s), 3):
        R.set_actors(eng, [R.constant_actor(b3s[i + a]) for a in range(3)])
        if not started:
            eng.reset()
            started = True
        la = R.Launch(eng, 2, False, quad)
        for a in range(3):
            want = np.broadcast_to(b3s[i + a], la.logits[:, :, a, :].shape)
            assert la.logits[:, :, a, :].tobytes() == np.ascontiguousarray(want).tobytes(), (i, a)
            assert (la.actions[:, :, a] == int(np.argmax(b3s[i + a]))).all(), (i, a, b3s[i + a])
            seen.add(tuple(np.unique(b3s[i + a], return_inverse=True)[1].tolist()))
        _mode_holds(la)
    assert seen == set(R.order_patterns())
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- b. the draws
@SHAPES
def test_draws_over_an_episode_and_into_the_next(N, quad):
    eng = R.engine(N, quad)
    R.set_actors(eng, [R.torch_actor(600 + a) for a in range(3)])
    eng.reset()
    tally = R.Tally()
    first = []
    for k in (40, 40, 16):
        la = R.Launch(eng, k, True, quad)
        assert (la.episode == 1).all()
        tally.check(la)
        first.append(la)
    # the auto-reset inside the last launch: every env is in its next episode, at step 0
    la = R.Launch(eng, 8, True, quad)
    assert (la.episode == 2).all() and la.step0 == 0
    tally.check(la)
    # ... whose draws are not the first episode's at the same steps: the restated uniforms differ, and the device's actions are not
    # what the first episode's uniforms give from the same logits
    u_old = first[0].u[:8]
    assert (u_old != la.u).mean() > 0.99
    old, unsure = R.draw_ref(la.logits, u_old)
    assert ((old != la.actions) & ~unsure).any()
    tally.close("episode + 8 steps, N = %d" % N)
    eng.close()


@SHAPES
def test_draws_key_on_the_global_env_index_and_the_whole_seed(N, quad):
    nets = [R.torch_actor(610 + a) for a in range(3)]
    tally = R.Tally()
    seen = []
    # env_index_base: a shard of a larger job draws its own envs' numbers
    eng = R.engine(N, quad, seed=5, env_index_base=R.BASE)
    R.set_actors(eng, nets)
    eng.reset()
    la = R.Launch(eng, 8, True, quad)
    tally.check(la)
    seen.append(la.u)
    assert (R.uniforms(5, 0, la.episode, la.steps) != la.u).mean() > 0.99
    eng.close()
    # the seed's high word; then another seed on the same engine
    eng = R.engine(N, quad, seed=R.HIGH_SEED)
    R.set_actors(eng, nets)
    eng.reset()
    la = R.Launch(eng, 8, True, quad)
    tally.check(la)
    seen.append(la.u)
    assert (R.uniforms(R.HIGH_SEED & 0xFFFFFFFF, 0, la.episode, la.steps) != la.u).mean() > 0.99
    other = (0xC2B2AE35 << 32) | 0x85EBCA6B
    eng.set_seed(other)
    eng.reset()
    assert eng.seed == other
    la = R.Launch(eng, 8, True, quad)
    assert (la.episode == 2).all() and la.step0 == 0
    tally.check(la)
    seen.append(la.u)
    assert (seen[1] != seen[2]).mean() > 0.99
    tally.close("env_index_base, 64-bit seed, set_seed, N = %d" % N)
    eng.close()


@SHAPES
def test_draws_with_episode_numbers_that_differ_inside_a_wavefront(N, quad):
    """a full reset, then a masked reset of every third env: the batch stays in lock-step (every env at episode step 0) while the
    envs of one wavefront -- two or four neighbours -- are in episodes 1 and 2"""
    eng = R.engine(N, quad, seed=9)
    R.set_actors(eng, [R.torch_actor(620 + a) for a in range(3)])
    eng.reset()
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    eng.reset(mask=mask)
    tally = R.Tally()
    la = R.Launch(eng, 12, True, quad)
    np.testing.assert_array_equal(la.episode, 1 + mask)
    per_wave = 4 if quad else 2
    assert all(len(set(la.episode[w:w + per_wave])) == 2 for w in range(0, N, per_wave) if mask[w:w + per_wave].any())
    tally.check(la)
    # (keyed on ONE episode number for all, the restated draws are others for the re-reset envs)
    assert (R.uniforms(9, 0, np.ones(N), la.steps)[:, mask == 1] != la.u[:, mask == 1]).mean() > 0.99
    tally.close("episodes 1 and 2 interleaved, N = %d" % N)
    eng.close()


@SHAPES
def test_draws_from_degenerate_and_skewed_distributions(N, quad):
    """w3 = 0, logits = b3: a distribution with all its mass on one action always draws it (its u = 0 included); (0, -200, 0) never
    draws 1 and splits 0 / 2 at u = 0.5 exactly; (0, -3, -6) and its rotations hold both thresholds away from symmetry.  The unsure
    share of these launches follows from Philox alone: tests/test_actor_ref.py holds it to the cap on the CPU for this seed."""
    eng = R.engine(N, quad, seed=R.CONSTANT_SEED)
    tally = R.Tally()
    for i, b3s in enumerate(R.CONSTANT_LAUNCHES):
        R.set_actors(eng, [R.constant_actor(b3) for b3 in b3s])
        if i == 0:
            eng.reset()
        la = R.Launch(eng, R.CONSTANT_K, True, quad)
        assert la.step0 == i * R.CONSTANT_K and (la.episode == 1).all()
        for a, b3 in enumerate(b3s):
            lg, got = la.logits[:, :, a, :], la.actions[:, :, a]
            assert lg.tobytes() == np.ascontiguousarray(np.broadcast_to(np.float32(b3), lg.shape)).tobytes(), (i, a)
            if b3 in R.ALWAYS:
                assert (got == R.ALWAYS[b3]).all(), (b3, np.bincount(got.ravel(), minlength=3))
            elif b3 == R.HALVES:
                np.testing.assert_array_equal(got, np.where(la.u[..., a] < 0.5, 0, 2))
                assert (got == 0).any() and (got == 2).any()
            else:
                tally.check(la, agents=(a,))
    assert abs(tally.share() - R.constant_unsure_share(N)) < 1e-12      # (the same number the CPU test holds)
    tally.close("constant logits, N = %d" % N)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- c. network paths
TOL = 2e-4      # tests/test_gpu_actor.py's bound for the same network with the feature LayerNorm on


def _logit_errors(la, nets):
    """-> (max |device - fp64|, max |torch fp32 - fp64|) over the launch, the networks on the observations the kernel saw"""
    import copy
    import torch
    inp = la.inputs()
    dev = f32 = 0.0
    for a in range(3):
        with torch.no_grad():
            ref64 = copy.deepcopy(nets[a]).double()(inp[:, :, a, :].double()).numpy()
            ref32 = nets[a](inp[:, :, a, :]).numpy()
        assert np.isfinite(ref64).all()
        dev = max(dev, float(np.abs(la.logits[:, :, a, :] - ref64).max()))
        f32 = max(f32, float(np.abs(ref32 - ref64).max()))
    return dev, f32


@SHAPES
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_network_without_the_feature_layernorm(N, quad, activation):
    """A state_dict without base.feature_norm.* (use_feature_normalization False in the reference): flags bit 0 clear, the padded
    observation goes to the first Linear as it is.  tanh: no agent normalises; relu: agent_dc alone does (the flag is per agent).
    Bound: the 2e-4 of tests/test_gpu_actor.py.  Measured on the MI355X: 3.2e-6 (tanh) and 3.4e-6 (relu) from torch fp64, where
    torch's own fp32 is 2.3e-6 and 3.1e-6 off."""
    import torch
    normed = (1,) if activation == "relu" else ()
    nets = [R.torch_actor(700 + a, activation, logit_scale=1.0, feature_norm=a in normed) for a in range(3)]
    eng = R.engine(N, quad)
    R.set_actors(eng, nets, activation)
    for a in range(3):
        assert eng._actors[a].use_feature_normalization == (1 if a in normed else 0)
    eng.reset()
    la = R.Launch(eng, 24, False, quad)
    dev, f32 = _logit_errors(la, nets)
    print("no feature LayerNorm (%s, N = %d): max |logit - fp64| %.2e (torch fp32 against fp64: %.2e)" % (activation, N, dev, f32))
    assert dev <= TOL, (dev, f32)
    # (the flag is live: WITH a feature LayerNorm of unit gain the same weights give other logits)
    a = 0
    with torch.no_grad():
        x = la.inputs()[:, :, a, :].double()
        m = nets[a].double()
        other = m.act.action_out.linear(m.base.mlp.fc(torch.nn.functional.layer_norm(x, (26,)))).numpy()
    assert np.abs(other - la.logits[:, :, a, :]).max() > 100 * TOL
    _mode_holds(la)
    eng.close()


@SHAPES
@pytest.mark.parametrize("dead", [1, 2])
def test_network_with_a_dead_relu_layer(N, quad, dead):
    """relu with w = 0, b = -1 in hidden layer `dead`: its activations are all 0, the LayerNorm behind it sees variance 0 and must
    return its beta exactly -- rsq(0 + eps) times a zero difference, not a NaN.  Layer 1 dead: the rest of the network runs on
    ln1_beta, bound as above.  Layer 2 dead: logits = w3 . ln2_beta + b3, and the bound is derived: 64 products of 2^-24 each and a
    six-level sum, inside 64 * 2^-23 * sum_j |w3[c][j] ln2_beta[j]| per logit.  Measured on the MI355X: layer 1 dead 1.4e-6 from torch
    fp64 (torch fp32: 1.3e-6); layer 2 dead 7.0e-8 against bounds of 1.4e-5 and more."""
    import torch
    nets = [R.torch_actor(800 + a, "relu", logit_scale=1.0) for a in range(3)]
    with torch.no_grad():
        for m in nets:
            lin = m.base.mlp.fc[0 if dead == 1 else 3]
            lin.weight.zero_()
            lin.bias.fill_(-1.0)
    eng = R.engine(N, quad)
    R.set_actors(eng, nets, "relu")
    eng.reset()
    la = R.Launch(eng, 8, False, quad)
    assert not np.isnan(la.logits).any()
    dev, f32 = _logit_errors(la, nets)
    print("dead layer %d (N = %d): max |logit - fp64| %.2e (torch fp32 against fp64: %.2e)" % (dead, N, dev, f32))
    assert dev <= TOL, (dev, f32)
    for a in range(3):
        lg = la.logits[:, :, a, :]
        assert (lg == lg[0, 0]).all()                  # (no observation reaches the logits)
        if dead == 2:
            w3 = nets[a].act.action_out.linear.weight.double().detach().numpy()
            b3 = nets[a].act.action_out.linear.bias.double().detach().numpy()
            beta = nets[a].base.mlp.fc[5].bias.double().detach().numpy()
            want = w3 @ beta + b3
            bound = 64 * 2.0 ** -23 * np.abs(w3 * beta).sum(-1)
            err = np.abs(lg[0, 0].astype(np.float64) - want)
            print("  agent %d: |logit - (w3 . ln2_beta + b3)| %s, bound %s" % (a, err, bound))
            assert (err <= bound).all(), (a, err, bound)
    _mode_holds(la)
    eng.close()
