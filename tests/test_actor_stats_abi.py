"""sdc_rollout_actor_stats on the CPU side: declared with its argument names, exported and bound with the ABI still at 313;
sdc_policy_stats.hip is one of the library's sources; the header's two #defines and enums are the binding's constants; the library refuses
a null handle before it touches a device; the translation unit cross-compiles for gfx950 with no scratch, no spills, no LDS and an
occupancy of at least 4 for exactly its one kernel; PolicyStats.summary() on hand-made CPU tensors against a NumPy restatement written out
here; EpisodeStats keeps its three-argument form."""
import re

import numpy as np

from dc_rl_amd import _lib as L
from tests.plan_util import assert_no_scratch_or_spills, entry_point_header, kernel_resources

ARGS = ["h", "n_steps", "sample", "accumulate", "stats", "returns", "counts", "policy_counts", "policy_sums", "obs", "share_obs", "rew",
        "done", "info", "final_obs", "stream"]


def test_actor_stats_entry_point_is_declared_exported_and_bound_at_abi_313():
    hdr = entry_point_header("sdc_rollout_actor_stats", ARGS, "sdc_policy_stats.hip")
    m = re.search(r"#define SDC_POLICY_COUNTS (\d+)", hdr)
    assert m and int(m.group(1)) == L.POLICY_COUNTS == 5
    m = re.search(r"#define SDC_POLICY_SUMS (\d+)", hdr)
    assert m and int(m.group(1)) == L.POLICY_SUMS == 2
    assert re.search(r"enum sdc_policy_count \{ SDC_POLICY_N0 = 0, SDC_POLICY_N1, SDC_POLICY_N2, SDC_POLICY_SWITCHES, SDC_POLICY_LAST \};", hdr)
    assert re.search(r"enum sdc_policy_sum \{ SDC_POLICY_LOGP = 0, SDC_POLICY_ENTROPY \};", hdr)
    assert (L.POLICY_N0, L.POLICY_N1, L.POLICY_N2, L.POLICY_SWITCHES, L.POLICY_LAST) == (0, 1, 2, 3, 4)
    assert (L.POLICY_LOGP, L.POLICY_ENTROPY) == (0, 1)
    import dc_rl_amd
    from dc_rl_amd.engine import PolicyStats, SdcEngine
    assert dc_rl_amd.PolicyStats is PolicyStats
    assert callable(SdcEngine.rollout_actor_stats)
    for nm in ("set_actor", "rollout_actor_stats", "evaluate"):
        assert callable(getattr(dc_rl_amd.SustainDCVecEnv, nm)), nm
    assert not hasattr(dc_rl_amd.SustainDCMultiDeviceVecEnv, "rollout_actor_stats")
    assert not hasattr(dc_rl_amd.SustainDCMultiDeviceVecEnv, "set_actor")


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_rollout_actor_stats(None, 1, 0, 0, *([None] * 12)) == -2
    assert b"sdc_rollout_actor_stats: null handle" in lib.sdc_last_error()


def test_policy_stats_kernel_compiles_for_gfx950_without_scratch_spills_or_lds():
    per = kernel_resources("sdc_policy_stats.hip")
    assert_no_scratch_or_spills(per, {"sdc_policy_stats_kernel"})
    u = per["sdc_policy_stats_kernel"]
    assert u["LDS Size"] == 0, u      # no LDS, as the kernel's header says
    assert u["Occupancy"] >= 4, u     # the bar the sibling reduce kernels are held to (tests/test_stats_abi.py)


def _summary_ref(counts, sums):
    """PolicyStats.summary restated: counts [..., N, 3, 5] (n0, n1, n2, switches, last), sums [..., N, 3, 2] (logp, entropy)"""
    n = counts[..., :3].astype(np.float64)
    steps = n[..., 0] + n[..., 1] + n[..., 2]                       # [..., N, 3]
    sw = counts[..., 3].astype(np.float64)
    trans = np.maximum(steps - 1.0, 1.0)
    env_axis = steps.ndim - 2
    tot = steps.sum(axis=env_axis)                                   # [..., 3]
    safe = np.where(steps > 0, steps, 1.0)
    tsafe = np.where(tot > 0, tot, 1.0)
    per_env = {
        "action_frequency": np.where(steps[..., None] > 0, n / safe[..., None], 0.0),
        "mean_entropy": np.where(steps > 0, sums[..., 1] / safe, 0.0),
        "mean_logp": np.where(steps > 0, sums[..., 0] / safe, 0.0),
        "switch_rate": sw / trans,
    }
    batch = {
        "action_frequency": np.where(tot[..., None] > 0, n.sum(axis=env_axis) / tsafe[..., None], 0.0),
        "mean_entropy": np.where(tot > 0, sums[..., 1].sum(axis=env_axis) / tsafe, 0.0),
        "mean_logp": np.where(tot > 0, sums[..., 0].sum(axis=env_axis) / tsafe, 0.0),
        "switch_rate": sw.sum(axis=env_axis) / trans.sum(axis=env_axis),
    }
    return per_env, batch, steps.astype(np.int64)


def _hand_made(rng, N):
    """counts / sums of N envs: env 0 took ONE step (no transition: switch rate 0 without a division by zero), env 1 none at all, the
    others 2 .. 40 steps with switches <= steps - 1"""
    counts = np.zeros((N, 3, 5), dtype=np.int32)
    sums = np.zeros((N, 3, 2), dtype=np.float64)
    for e in range(N):
        for a in range(3):
            steps = 1 if e == 0 else (0 if e == 1 else int(rng.integers(2, 41)))
            split = np.sort(rng.integers(0, steps + 1, size=2))
            counts[e, a, :3] = [split[0], split[1] - split[0], steps - split[1]]
            counts[e, a, 3] = 0 if steps < 2 else int(rng.integers(0, steps))
            counts[e, a, 4] = -1 if steps == 0 else int(rng.integers(0, 3))
            sums[e, a] = [-steps * rng.uniform(0.05, 1.5), steps * rng.uniform(0.0, np.log(3.0))]
    return counts, sums


def _check(got, per_env, batch, steps):
    assert set(got) == {"per_env", "batch", "steps"}
    assert set(got["per_env"]) == set(per_env) and set(got["batch"]) == set(batch)
    for k in per_env:
        assert got["per_env"][k].dtype == np.float64 and got["per_env"][k].shape == per_env[k].shape, k
        assert np.array_equal(got["per_env"][k], per_env[k]), k
        assert np.asarray(got["batch"][k]).shape == batch[k].shape, k
        assert np.array_equal(got["batch"][k], batch[k]), k
    assert np.array_equal(got["steps"], steps)


def test_policy_stats_summary_against_a_numpy_restatement():
    import torch
    from dc_rl_amd import PolicyStats
    rng = np.random.default_rng(11)
    N = 6
    counts, sums = _hand_made(rng, N)
    ps = PolicyStats(torch.from_numpy(counts), torch.from_numpy(sums))
    # the views
    assert ps.action_counts.shape == (N, 3, 3) and torch.equal(ps.action_counts, ps.counts[:, :, :3])
    assert torch.equal(ps.switches, ps.counts[:, :, 3]) and torch.equal(ps.last_action, ps.counts[:, :, 4])
    assert torch.equal(ps.logp, ps.sums[:, :, 0]) and torch.equal(ps.entropy, ps.sums[:, :, 1])
    assert ps.logp.data_ptr() == ps.sums.data_ptr()      # views, not copies
    got = ps.summary()
    per_env, batch, steps = _summary_ref(counts, sums)
    _check(got, per_env, batch, steps)
    assert got["per_env"]["action_frequency"].shape == (N, 3, 3) and got["batch"]["switch_rate"].shape == (3,)
    # the env with one step: a frequency of 1 on its action, switch rate 0; the env with none: zeros, nothing NaN
    assert np.array_equal(got["per_env"]["switch_rate"][0], np.zeros(3)) and np.array_equal(got["per_env"]["action_frequency"][0].sum(-1), np.ones(3))
    assert np.array_equal(got["per_env"]["action_frequency"][1], np.zeros((3, 3))) and np.array_equal(got["per_env"]["mean_logp"][1], np.zeros(3))
    assert all(np.isfinite(v).all() for v in got["per_env"].values()) and all(np.isfinite(v).all() for v in got["batch"].values())
    # a leading [E] dimension, as from evaluate
    c2, s2 = _hand_made(rng, N)
    pe = PolicyStats(torch.from_numpy(np.stack([counts, c2])), torch.from_numpy(np.stack([sums, s2])))
    got = pe.summary()
    per_env, batch, steps = _summary_ref(np.stack([counts, c2]), np.stack([sums, s2]))
    _check(got, per_env, batch, steps)
    assert got["per_env"]["mean_entropy"].shape == (2, N, 3) and got["batch"]["action_frequency"].shape == (2, 3, 3)
    first = ps.summary()
    for k in first["batch"]:
        assert np.array_equal(got["batch"][k][0], first["batch"][k]), k


def test_episode_stats_keeps_its_three_argument_form():
    import torch
    from dc_rl_amd import EpisodeStats, PolicyStats
    stats, ret, cnt = torch.zeros((4, 2, L.INFO_DIM), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.float64), torch.ones((2, 2), dtype=torch.int32)
    st = EpisodeStats(stats, ret, cnt)
    assert st.policy is None and st.stats is stats and st.returns is ret and st.counts is cnt
    assert set(st.summary()) == {"per_env", "batch", "steps", "fault"}
    ps = PolicyStats(torch.zeros((2, 3, 5), dtype=torch.int32), torch.zeros((2, 3, 2), dtype=torch.float64))
    assert EpisodeStats(stats, ret, cnt, ps).policy is ps
