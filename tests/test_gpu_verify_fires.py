"""Verify mode (debug_flags DEBUG_VERIFY: csrc/sdc_verify.hip behind every step) FIRES.  Some twenty GPU tests end with
`order_stat_sticky == 0` / `info[fault] == 0`; this one shows that the kernel behind those lines can raise SDC_FAULT_ORDER_STAT and set
the sticky bit -- on every step mapping, in the right info row, for the corruptions of tests/verify_cases.py written into a REAL
reward state -- and that it stays silent for the clean envs beside them.

Two engines with the same seed, 256 envs, hist_cap 10 000, 16-step episodes, no auto-reset; rings injected before the first reset
(331 + 70 N(0, 1), clipped to 100 .. 650 -- tests/test_gpu_wide.py clips at 150, which leaves no key below the lower clip bound and so
nothing for kind 4 to count down).  History lengths when the corruption is written, by env // 64: 10 000 (every step evicts), 1 500,
33 .. 100 mixed, 30 (31 at the step that is asserted: below SMALL_N the trackers are not used and the verify kernel returns early;
the five steps after it cross SMALL_N and build the state).  One whole episode builds every env's reward state; between the episodes
engine A gets the corrupted header / qwin, engine B its own bytes back (the same side effects of set_state); both are reset -- the
reset keeps the reward state and rebuilds the feature rows, so the specialised kernels run -- and stepped with the same actions.

At the first step after the write:
  clean       no fault bit, sticky 0, all five outputs bit-equal to B's (info[reserved] aside); B raises nothing anywhere
  must fire   every env whose step was served from the incremental state alone (info[reserved] == 0) shows SDC_FAULT_ORDER_STAT and
              the sticky bit; at least half of each kind's envs of 32 or more keys are such envs
  otherwise   (healed, either, a must-fire env on another path) the fault bit, OR info[energy_z] agrees with an fp64 NumPy z from the
              state read back after the step within the kernel's own 2e-6 |z| + 1e-6: no silently wrong z.  Kinds 12 and 13
              rebuild (info[reserved] == 3) without a fault.
Five more steps: order_stat_sticky is 1 exactly for the envs that ever showed the bit; a step that rebuilt an env (path 3) shows no
bit for it.  The sticky bit lives in the header, of which a reset clears the episode returns alone (csrc/sdc_reset.hip): it survives
reset() and is cleared only by writing the header.

Checks of the kernel that no injection reaches: DESIGN.md section 4.1.1."""
import os
import re

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from dc_rl_amd import dc_config, traces
from dc_rl_amd.engine import SdcEngine
from tests import verify_cases as VC
from tests.gpu_helpers import hdr_offsets

pytestmark = pytest.mark.gpu

N, CAP, EP = 256, 10000, 16
MAPPINGS = {      # debug_flags override, data-centre config, the kernel it must land on
    "general": (L.DEBUG_GENERAL, "dc_config.json", "sdc_dynamics_kernel"),
    "pair": (L.DEBUG_PAIR, "dc_config.json", "sdc_dynamics_fast_kernel"),
    "quad": (L.DEBUG_QUAD, "dc_config.json", "sdc_dynamics_quad_kernel"),
    "wide": (L.DEBUG_WIDE, "dc_config.json", "sdc_dynamics_wide_kernel"),
    "wide_gen": (L.DEBUG_WIDE, "dc_config_r25.json", "sdc_dynamics_wide_gen_kernel"),      # (11 rack classes: tests/test_gpu_wide_gen.py)
}


def fault_order_stat():
    src = open(os.path.join(os.path.dirname(L.CSRC), os.pardir, "include", "sustaindc_hip.h")).read()
    return int(re.search(r"#define SDC_FAULT_ORDER_STAT (\d+)u", src).group(1))


def lengths_at_write():
    e = np.arange(N)
    return np.select([e < 64, e < 128, e < 192], [CAP, 1500, 33 + (e * 7) % 68], 30)


@pytest.fixture(scope="module")
def rings():
    """the injected rings: shared by every mapping, never written to"""
    rng = np.random.default_rng(2024)
    n0 = np.where(lengths_at_write() == CAP, CAP, lengths_at_write() - EP)      # an episode appends EP keys to a ring that is not full
    hist = np.full((N, 10240), np.nan, np.float32)
    vals = (331 + 70 * rng.standard_normal((N, CAP))).clip(100, 650).astype(np.float32)
    for e in range(N):
        hist[e, :n0[e]] = vals[e, :n0[e]]
    pos = np.where(n0 == CAP, rng.integers(0, CAP, N), 0).astype(np.int32)
    hist.setflags(write=False)
    return hist, n0.astype(np.int32), pos


def engines(flag, cfg, rings):
    hist, n0, pos = rings
    tb = traces.synthetic_tables("ny", 0)
    p = dc_config.size_datacenter(cfg, 1, 30.0)
    out = []
    for _ in range(2):
        e = SdcEngine(N, episode_steps=EP, auto_reset=False, seed=77, hist_cap=CAP, debug_flags=L.DEBUG_VERIFY | flag)
        e.set_tables(0, tb["W"], tb["C"], tb["T"], tb["WB"])
        e.set_dc_params(0, p)
        e.assign(0, 0, 200, 210)
        e.set_state("hist", hist)
        e.set_state("hist_len", n0)
        e.set_state("hist_pos", pos)
        e.reset()
        out.append(e)
    return out


def outputs(eng, acts):
    """the five outputs of a step on the host, info[reserved] apart"""
    rsv = L.INFO_IDX["reserved"]
    o = [x.cpu().numpy().copy() for x in eng.step(acts)]
    path = o[4][:, rsv].astype(np.int64)
    o[4][:, rsv] = 0
    return o, path


@pytest.mark.parametrize("mapping", list(MAPPINGS))
def test_corrupted_reward_state_raises_the_fault_on_every_step_mapping(mapping, rings):
    import torch
    flag, cfg, kernel = MAPPINGS[mapping]
    BIT = fault_order_stat()
    H = VC.offsets(hdr_offsets(), open(os.path.join(L.CSRC, "sdc_device.hpp")).read())
    fcol, zcol = L.INFO_IDX["fault"], L.INFO_IDX["energy_z"]
    a, b = engines(flag, cfg, rings)
    try:
        g = torch.Generator(device="cpu").manual_seed(41)
        acts = torch.randint(0, 3, (EP + 6, N, 3), dtype=torch.int32, generator=g).cuda()
        # 1. one whole episode: every env of 32 or more keys holds a built reward state
        for t in range(EP):
            a.step(acts[t])
            b.step(acts[t])
        for e in (a, b):
            assert (e.info[:, fcol] == 0).all() and (e.get_state("order_stat_sticky") == 0).all()
        # 2. the state between the episodes; 3. the corruption into A, B's own bytes back into B
        header, qwin, hist = a.get_state("header"), a.get_state("qwin"), a.get_state("hist")
        assert np.array_equal(header[:, H["H_N"]], lengths_at_write())
        res = VC.corrupt(header, qwin, hist, H)
        big = res.n >= 1500
        assert not [d for d in res.demoted if big[d[0]]], res.demoted      # none may be left out among the long histories
        print(f"\n[{mapping}] kinds that could not be placed (env, kind, why):", res.demoted)
        a.set_state("header", res.header)
        a.set_state("qwin", res.qwin)
        b.set_state("header", b.get_state("header"))
        b.set_state("qwin", b.get_state("qwin"))
        # 4. reset both; 5. step both
        a.reset()
        b.reset()
        (oa, path), (ob, path_b) = outputs(a, acts[EP]), outputs(b, acts[EP])
        assert a.last_step_kernel() == kernel and b.last_step_kernel() == kernel
        fa, fb = oa[4][:, fcol].astype(np.int64), ob[4][:, fcol].astype(np.int64)
        sticky, sticky_b = a.get_state("order_stat_sticky"), b.get_state("order_stat_sticky")
        fired = (fa & BIT) != 0
        assert ((fa & ~BIT) == 0).all() and (fb == 0).all() and (sticky_b == 0).all()      # B raises nothing anywhere
        assert np.array_equal(sticky != 0, fired)                                          # the bit and the sticky bit go together
        hdr1, hist1 = a.get_state("header"), a.get_state("hist")
        n1 = hdr1[:, H["H_N"]].astype(np.int64)
        assert np.array_equal(n1, np.minimum(lengths_at_write() + 1, CAP))
        z_ref = np.array([VC.z_reference(hist1[e], VC.get_f64(hdr1[e], H["H_EOFF"])) for e in range(N)])
        z_ok = np.abs(oa[4][:, zcol].astype(np.float64) - z_ref) <= VC.z_tol(z_ref)
        # the census: per kind, how the envs of 32 or more keys were served and what the kernel said
        census = {}
        for k in range(16):
            m = (res.kind == k) & (res.wanted == k) & (n1 >= VC.SMALL_N)      # (an env whose kind could not be placed counts nowhere)
            census[k] = dict(envs=int(m.sum()), paths={int(p): int(((path == p) & m).sum()) for p in np.unique(path[m])},
                             fired=int((fired & m).sum()), fired_path0=int((fired & m & (path == 0)).sum()), z_ok=int((z_ok & m).sum()))
        for k in range(16):
            print(f"[{mapping}] kind {k:2d} {VC.NAME_OF_KIND[k]:22s} {VC.CLASS_OF_KIND[k]:9s} {census[k]}")
        print(f"[{mapping}] twin's paths:", {int(p): int((path_b == p).sum()) for p in np.unique(path_b)})
        # clean: controls, demoted envs, every env below SMALL_N whatever was written into it
        clean = res.cls == VC.CLEAN
        assert clean[n1 < VC.SMALL_N].all() and (n1 < VC.SMALL_N).sum() == 64
        assert not fired[clean].any(), np.flatnonzero(fired & clean)
        for u, v, nm in zip(oa, ob, ("obs", "share_obs", "rew", "done", "info")):
            same = (u[clean] == v[clean]) | ((u[clean] != u[clean]) & (v[clean] != v[clean]))
            assert same.all(), (nm, np.flatnonzero(clean)[np.argwhere(~same)[:4, 0]])
        assert z_ok[clean].all()      # (and the reference agrees with the device where nothing was touched)
        # must fire
        must = res.cls == VC.MUST_FIRE
        silent = must & (path == 0) & ~fired
        assert not silent.any(), [(int(e), int(res.kind[e])) for e in np.flatnonzero(silent)]
        for k in (k for k, c in VC.CLASS_OF_KIND.items() if c == VC.MUST_FIRE):
            assert census[k]["paths"].get(0, 0) >= 6, (k, census[k])
        # healed, either, and the must-fire envs another path served: the bit, or a z that is right
        rest = ~clean & ~(must & (path == 0))
        wrong = rest & ~fired & ~z_ok
        assert not wrong.any(), [(int(e), int(res.kind[e]), int(path[e])) for e in np.flatnonzero(wrong)]
        healed = res.cls == VC.HEALED
        assert healed.sum() == 2 * 12 and (path[healed] == 3).all() and not fired[healed].any()
        # 6. five more steps: the sticky bit is the OR of what info showed; a rebuilt env is clean in that step
        ever = fired.copy()
        for t in range(EP + 1, EP + 6):
            (oa, path), (ob, _) = outputs(a, acts[t]), outputs(b, acts[t])
            f = (oa[4][:, fcol].astype(np.int64) & BIT) != 0
            assert (ob[4][:, fcol] == 0).all()
            assert not f[path == 3].any(), (t, np.flatnonzero(f & (path == 3)))
            assert not f[clean].any(), (t, np.flatnonzero(f & clean))
            ever |= f
        assert np.array_equal(a.get_state("order_stat_sticky") != 0, ever)
        assert (b.get_state("order_stat_sticky") == 0).all()
        assert not f[healed].any()
        print(f"[{mapping}] envs that ever showed the bit: {int(ever.sum())}; still showing it after six steps: {int(f.sum())}")
        # ... and across the next reset: the header keeps it (a reset clears the episode returns alone)
        for t in range(EP + 6, 2 * EP):
            x = acts[t % (EP + 6)]
            a.step(x)
            b.step(x)
            ever |= (a.info[:, fcol].cpu().numpy().astype(np.int64) & BIT) != 0
        a.reset()
        assert np.array_equal(a.get_state("order_stat_sticky") != 0, ever)
    finally:
        a.close()
        b.close()
