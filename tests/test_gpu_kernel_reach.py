"""The step kernels at the edges of their reach (csrc/sdc_dispatch.hpp: sdc_single_step_path / sdc_rollout_path decide which kernel a
call lands on; tests/test_step_dispatch.py holds those functions to the same tables without a GPU):

  * batch sizes either side of every threshold, each in the production configuration (tests/production_rig.py: debug_flags 0, full
    rings, one auto-reset, the kernel's own geometry sampled against the oracle) -- and WHICH kernel each lands on, from a table
    (tests/step_paths.py KERNEL_OF_BATCH) that must be edited on purpose when a threshold moves;
  * rack counts 1 / 17 / 31 / 32 / 33 and configs of exactly 8 / 9 / 12 / 13 rack classes, on every mapping each is eligible for
    (forced by debug_flags), every env the same bits as the general kernel, sampled envs against the oracle, and where each lands;
  * the two mirrors the lane-per-env kernel reads -- the ring's slot-major copy (SdcDev::hist_t, 49 152 envs and up) and the queue
    table's time-major copy (qcum_t, 7 680 envs and up) -- kept coherent by the OTHER kernels: a batch that switches between the
    general kernel (`step(want_info=False)`: no specialised kernel runs without `info`) and the lane-per-env kernel, held bit for bit
    to a batch that never leaves the four-envs-per-wavefront kernel;
  * sdc_rollout on every kernel it can land on (forced by debug_flags, by `actions_out`, by the batch's size modulo 2 and 4), every
    output the same bits as the general multi-step kernel's."""
import json
import os

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import dc_config
from tests.production_rig import ProductionRig
from tests.step_paths import GENERAL, KERNEL_OF_BATCH, PAIR, QUAD, RACK_CASES, ROLLOUT_CASES, WIDE, WIDE_OFF, expected_mapping

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("N", sorted(KERNEL_OF_BATCH))
def test_batch_size_thresholds_production_vs_oracle(N):
    mapping = KERNEL_OF_BATCH[N]
    rig = ProductionRig(N, mapping, debug_flags=0, episode_steps=64, seed=7000 + N, n_random=24)
    obs, _ = rig.eng.reset()
    rig.begin_all(obs)
    rig.single_steps(72)       # (the first step asserts the kernel the sample was built for)
    print(f"{N} envs: {rig.eng.last_step_kernel()} worst {rig.worst} sampled {len(rig.sample)} auto-resets {rig.resets}")
    assert rig.eng.last_step_kernel() == rig.geom.kernel and rig.resets == 1
    rig.assert_ok()
    rig.eng.close()


def rack_config(tmp_path, n_racks, n_classes=None):
    """dc_config.json with n_racks racks in one row.  n_classes None: the shipped per-rack lists repeated (the test of
    tests/test_gpu_stagger.py::test_odd_batch_and_more_than_32_racks_vs_oracle); else every rack the same servers and exactly
    n_classes distinct supply approach temperatures (a rack class = CPUs, supply approach, full / idle power: SdcRackClasses)."""
    src = os.path.join(os.path.dirname(dc_config.__file__), "configs", "dc_config.json")
    cfg = json.load(open(src))
    d, sv = cfg["data_center_configuration"], cfg["server_characteristics"]
    d["NUM_ROWS"], d["NUM_RACKS_PER_ROW"] = 1, n_racks
    rep = lambda xs: (xs * (n_racks // len(xs) + 1))[:n_racks]
    if n_classes is None:
        d["RACK_SUPPLY_APPROACH_TEMP_LIST"] = rep(d["RACK_SUPPLY_APPROACH_TEMP_LIST"])
        d["RACK_RETURN_APPROACH_TEMP_LIST"] = rep(d["RACK_RETURN_APPROACH_TEMP_LIST"])
        sv["DEFAULT_SERVER_POWER_CHARACTERISTICS"] = rep(sv["DEFAULT_SERVER_POWER_CHARACTERISTICS"])
    else:
        d["RACK_SUPPLY_APPROACH_TEMP_LIST"] = [5.0 + 0.1 * (r % n_classes) for r in range(n_racks)]
        d["RACK_RETURN_APPROACH_TEMP_LIST"] = [-2.5] * n_racks
        sv["DEFAULT_SERVER_POWER_CHARACTERISTICS"] = [[130, 10]] * n_racks
    path = str(tmp_path / f"dc_config_r{n_racks}_c{n_classes}.json")
    json.dump(cfg, open(path, "w"))
    return path


def rack_classes(p):
    return len({(p["rack_n"][r], p["rack_supply"][r], p["rack_full"][r], p["rack_idle"][r]) for r in range(len(p["rack_n"]))})


def _same(ref, other, t, what):
    import torch
    rsv = L.INFO_IDX["reserved"]
    for nm, u, v in zip(("obs", "share_obs", "rew", "done", "info", "final_obs"),
                        (ref.obs, ref.share_obs, ref.rew, ref.done, ref.info, ref.final_obs),
                        (other.obs, other.share_obs, other.rew, other.done, other.info, other.final_obs)):
        if nm == "info":
            u, v = u.clone(), v.clone()
            u[:, rsv] = 0
            v[:, rsv] = 0
        if not torch.equal(u, v):
            bad = (u != v).nonzero()
            raise AssertionError((what, t, nm, bad[:6].tolist(), u[tuple(bad[0])].item(), v[tuple(bad[0])].item()))


@pytest.mark.parametrize("racks,classes", RACK_CASES)
def test_rack_counts_and_classes_on_every_eligible_mapping(tmp_path, racks, classes):
    """256 envs of one config (and 256 of it beside the shipped 20-rack config, for the lane-per-env kernel's general form) in the
    production configuration, 72 steps over an auto-reset: the general kernel's sampled envs against the oracle, every other mapping
    every env the same bits as the general kernel, final observations and rings included."""
    import torch
    path = rack_config(tmp_path, racks, classes)
    p = dc_config.size_datacenter(path, 1, 30.0)
    assert len(p["rack_n"]) == racks
    k = rack_classes(p)
    if classes is not None:
        assert k == classes
    N, steps, seed = 256, 64, 9000 + racks * 16 + (classes or 0)
    kw = dict(episode_steps=steps, seed=seed, n_random=24)
    groups = []
    for files in ((path,), (path, "dc_config.json")):
        two = len(files) == 2
        flags = (GENERAL, WIDE) if two else (GENERAL, PAIR, QUAD, WIDE, WIDE_OFF)
        rigs = [ProductionRig(N, expected_mapping(f, racks, k, two), debug_flags=f, dc_files=files, oracles=(f == GENERAL), **kw)
                for f in flags]
        groups.append(rigs)
    for rigs in groups:
        for r in rigs:
            obs, _ = r.eng.reset()
            r.begin_all(obs)
        g = torch.Generator(device="cpu").manual_seed(seed)
        for t in range(72):
            acts = torch.randint(0, 3, (N, 3), dtype=torch.int32, generator=g).cuda()
            for r in rigs:
                r.step(acts)       # (the first step asserts the expected kernel)
            for r in rigs[1:]:
                _same(rigs[0].eng, r.eng, t, (racks, k, r.eng.last_step_kernel()))
        ring = rigs[0].eng.get_state("hist").view(np.uint32)
        for r in rigs:
            assert r.resets == 1
            np.testing.assert_array_equal(ring, r.eng.get_state("hist").view(np.uint32))
        rigs[0].assert_ok()
        landed = [r.eng.last_step_kernel() for r in rigs]
        print(f"{racks} racks, {k} classes, {len(rigs[0].params)} config(s): worst {rigs[0].worst},", landed)
        assert landed == [r.geom.kernel for r in rigs]
        if racks > 32:
            assert set(landed) == {"sdc_dynamics_kernel"}, landed     # whatever the flags
        for r in rigs:
            r.eng.close()


@pytest.mark.parametrize("N", [7680, 49152])
def test_mirrors_stay_coherent_across_kernel_switches(N):
    """A batch that switches kernels between steps: blocks of `step(want_info=False)` (the general kernel: it appends to the ring,
    the queue table and their mirrors) between blocks of lane-per-env steps (which read the mirrors), against a second engine on
    the four-envs-per-wavefront kernel throughout -- obs, share_obs, rew, done (and final_obs, and info where both wrote it) the same
    bits over 300 steps and two auto-resets, the rings equal at the end.  The rings hold 128 keys, so that a key appended by the
    general kernel is EVICTED -- read from the mirror by the lane-per-env kernel -- within the test (10 000-key rings would not wrap)."""
    import torch
    cap = 128
    a = ProductionRig(N, "wide", debug_flags=0, episode_steps=120, seed=4900 + N, n_random=0, oracles=False, hist_cap=cap)
    b = ProductionRig(N, "quad", debug_flags=WIDE_OFF, episode_steps=120, seed=4900 + N, n_random=0, oracles=False, hist_cap=cap)
    for r in (a, b):
        obs, _ = r.eng.reset()
        r.begin_all(obs)
    g = torch.Generator(device="cpu").manual_seed(N)
    rsv = L.INFO_IDX["reserved"]
    switched = 0
    for t in range(300):
        acts = torch.randint(0, 3, (N, 3), dtype=torch.int32, generator=g).cuda()
        general = t % 11 >= 6            # six lane-per-env steps, then five on the general kernel
        a.step(acts, want_info=not general)
        assert a.eng.last_step_kernel() == ("sdc_dynamics_kernel" if general else "sdc_dynamics_wide_kernel"), t
        b.step(acts)
        switched += general
        for nm in ("obs", "share_obs", "rew", "done", "final_obs") + (() if general else ("info",)):
            u, v = getattr(a.eng, nm), getattr(b.eng, nm)
            if nm == "info":
                u, v = u.clone(), v.clone()
                u[:, rsv] = 0
                v[:, rsv] = 0
            if not torch.equal(u, v):
                bad = (u != v).nonzero()
                raise AssertionError((t, general, nm, bad[:6].tolist(), u[tuple(bad[0])].item(), v[tuple(bad[0])].item()))
    assert a.resets == b.resets == 2 and switched > 100
    np.testing.assert_array_equal(a.eng.get_state("hist").view(np.uint32), b.eng.get_state("hist").view(np.uint32))
    print(f"{N} envs: {switched} general-kernel steps among 300, auto-resets {a.resets}")
    for r in (a, b):
        r.eng.close()


@pytest.mark.parametrize("N", sorted({c[0] for c in ROLLOUT_CASES}))
def test_rollout_lands_on_each_multi_step_mapping_with_the_general_kernels_bits(N):
    """sdc_rollout, K = 3, 24-step episodes, nine calls (the eighth ends the episode: an auto-reset inside its last step): under each
    of tests/step_paths.py ROLLOUT_CASES the call lands on the kernel listed there, and obs, share_obs, rew, done, info (without
    info[reserved]: which way the step's reward state was served, a diagnostic that differs between a multi-step launch and single-step
    launches) and final_obs are the same bits as those of an engine held to the general multi-step kernel; `actions_out`, where given,
    is the actions applied."""
    import torch
    from dc_rl_amd import traces
    from dc_rl_amd.engine import SdcEngine
    steps, K = 24, 3
    cases = [c for c in ROLLOUT_CASES if c[0] == N]
    tb = traces.synthetic_tables("ny", 0)
    p = dc_config.size_datacenter("dc_config.json", 1, 30.0)
    engs = []
    for flags in [GENERAL] + [c[1] for c in cases]:
        e = SdcEngine(N, episode_steps=steps, auto_reset=True, seed=31, debug_flags=flags)
        e.set_tables(0, tb["W"], tb["C"], tb["T"], tb["WB"])
        e.set_dc_params(0, p)
        e.assign(0, 0, 200, 210)
        e.reset()
        engs.append(e)
    ref = engs[0]
    g = torch.Generator(device="cpu").manual_seed(N)
    acts = torch.randint(0, 3, (9 * K, N, 3), dtype=torch.int32, generator=g).cuda()
    rsv = L.INFO_IDX["reserved"]
    names = ("obs", "share_obs", "rew", "done", "info")
    ended = 0
    for r in range(9):
        seq = acts[r * K:(r + 1) * K].contiguous()
        want = ref.rollout(seq)
        assert ref.last_step_kernel() == "sdc_rollout_kernel"
        want[4][:, :, rsv] = 0
        ended += int(bool(want[3][-1].all()))
        for e, (_, flags, want_actions, kernel) in zip(engs[1:], cases):
            got = e.rollout(seq, want_actions=want_actions)
            assert e.last_step_kernel() == kernel, (N, flags, want_actions, r, e.last_step_kernel())
            got[4][:, :, rsv] = 0
            for nm, u, v in zip(names + ("final_obs",), tuple(want[:5]) + (ref.final_obs,), tuple(got[:5]) + (e.final_obs,)):
                assert torch.equal(u, v), (N, flags, want_actions, r, nm)
            if want_actions:
                assert torch.equal(got[5], seq), (N, flags, r, "actions_out")
    assert ended == 1
    for e in engs:
        assert (e.info[:, L.INFO_IDX["fault"]] == 0).all()
        e.close()
