"""The throughput regime: the batch sizes README / DESIGN section 4.7 / bench `secondary.batch_scan` quote 1.82-1.89 G env-steps/s at.

At 262 144 envs the lane-per-env kernel (sdc_wide.hip) runs four dispatch rounds, reads the key a step evicts from the ring's
slot-major mirror (SdcDev::hist_t: 10.5 GB) and its sweeps compete with env workgroups -- none of which the 65 536-env tests reach:
  * 262 144 envs against the fp64 oracle in the production configuration (tests/production_rig.py: the kernel's own geometry sampled,
    the device's reset draws held to their NumPy restatement with a non-zero env_index_base);
  * 131 072 envs, EVERY env: the lane-per-env kernel against the four-envs-per-wavefront kernel bit for bit over an auto-reset, and
    the rings at the end.
Host memory: a batch's rings are injected from ONE [N, 10240] fp32 buffer filled block by block (10.7 GB at 262 144 envs; the
library converts it into a key array of the same size), only the sampled envs' rings are kept; per step only the sampled rows
travel to the host (fault column and path histogram reduced on the device).  Each test prints its peak host RSS."""
import resource

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests.production_rig import ProductionRig

pytestmark = pytest.mark.gpu


def _peak_rss_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20     # (Linux: KiB)


def test_262144_envs_production_vs_oracle():
    """262 144 envs on the lane-per-env kernel, debug_flags 0, full 10 000-entry rings with duplicates, 150 single steps over an
    auto-reset: the first / last workgroups, both sides of every occupancy round (four rounds of 1024 workgroups) and a random spread
    against the oracle; every reward-state path seen."""
    N = 262144
    rig = ProductionRig(N, "wide", debug_flags=0, episode_steps=120, seed=262144, n_random=64, env_index_base=1 << 20)
    obs, _ = rig.eng.reset()
    rig.begin_all(obs)
    rig.single_steps(150)
    print(f"262144 envs: {rig.eng.last_step_kernel()} worst {rig.worst} reward-state paths {rig.paths[:4].tolist()} auto-resets "
          f"{rig.resets} sampled envs {len(rig.sample)} draws checked {rig.draws_checked} peak host RSS {_peak_rss_gb():.1f} GB")
    assert rig.eng.last_step_kernel() == "sdc_dynamics_wide_kernel" and rig.resets >= 1
    rig.assert_ok()
    rig.assert_all_reward_state_paths_seen()
    rig.eng.close()


def test_131072_envs_lane_per_env_equals_four_per_wavefront_for_every_env():
    """Two engines of 131 072 envs, the same seed, debug_flags 0 (lane per env, the ring's mirror) against DEBUG_WIDE_OFF (four envs per
    wavefront): 150 steps over an auto-reset, every output of every env the same bits (the diagnostics column aside: it says which
    path served the reward state), final observations included, and at the end the rings."""
    import torch
    N = 131072
    a = ProductionRig(N, "wide", debug_flags=0, episode_steps=120, seed=1310, n_random=0, oracles=False)
    b = ProductionRig(N, "quad", debug_flags=L.DEBUG_WIDE_OFF, episode_steps=120, seed=1310, n_random=0, oracles=False)
    a.eng.reset()
    b.eng.reset()
    g = torch.Generator(device="cpu").manual_seed(1310)
    rsv = L.INFO_IDX["reserved"]
    resets = 0
    for t in range(150):
        acts = torch.randint(0, 3, (N, 3), dtype=torch.int32, generator=g).cuda()
        outs = []
        for r in (a, b):
            outs.append(r.eng.step(acts))
            if t == 0:
                r.check_kernel()
        for u, v, nm in zip(outs[0], outs[1], ("obs", "share_obs", "rew", "done", "info")):
            if nm == "info":
                u, v = u.clone(), v.clone()
                u[:, rsv] = 0
                v[:, rsv] = 0
            if not torch.equal(u, v):
                bad = (u != v).nonzero()
                raise AssertionError((t, nm, bad[:6].tolist(), u[tuple(bad[0])].item(), v[tuple(bad[0])].item()))
        if bool(a.eng.done.any()):
            resets += 1
            assert torch.equal(a.eng.final_obs, b.eng.final_obs), t
    assert resets >= 1
    assert a.eng.last_step_kernel() == "sdc_dynamics_wide_kernel" and b.eng.last_step_kernel() == "sdc_dynamics_quad_kernel"
    for r in (a, b):
        assert not bool((r.eng.info[:, L.INFO_IDX["fault"]] != 0).any())
    ha = a.eng.get_state("hist")
    assert np.array_equal(ha.view(np.uint32), b.eng.get_state("hist").view(np.uint32))
    del ha
    print(f"131072 envs, every env: {resets} auto-reset(s), peak host RSS {_peak_rss_gb():.1f} GB")
    for r in (a, b):
        r.eng.close()
