"""The host's copy of the per-env facts (csrc/sdc_mirror.hpp) against the device's truth, across the entry points that read or write it:
reset, step, masked reset, clone, snapshot / restore into other envs, mark / step / rewind, and rollouts that end an episode -- with
auto_reset on and off.  8 envs of 12-step episodes, two data-centre configs and two locations assigned alternately.  After every call:
  * a whole-batch snapshot's manifest (what the host believes) == get_state("t_rel" / "cfg_id" / "loc_id") (what the device holds),
  * steps_to_episode_end() == 12 - max(t_rel),
  * last_done() == the envs that reached step 12 in the call,
  * last_step_kernel() names a specialised kernel exactly when all envs were at one episode step before the call (the batch meets the
    other conditions of tests/step_paths.py throughout: an even number of envs, feature rows, every config <= 32 racks, info wanted)."""
import numpy as np
import pytest

from dc_rl_amd import dc_config, traces
from dc_rl_amd.engine import SdcEngine
from tests.step_paths import KERNEL_NAME

pytestmark = pytest.mark.gpu

N, EP = 8, 12
SNAP_T_REL, SNAP_CFG_ID, SNAP_LOC_ID = 5, 7, 8      # include/sustaindc_hip.h enum sdc_snapshot_manifest
ROLLOUT_NAME = {"pair": "sdc_rollout_fast_kernel", "general": "sdc_rollout_kernel"}


class _Rig:
    def __init__(self, auto_reset):
        import torch
        self.torch = torch
        self.auto = auto_reset
        e = SdcEngine(N, episode_steps=EP, auto_reset=auto_reset, seed=11, n_locations=2, n_dc_configs=2)
        for loc, name in enumerate(("ny", "az")):
            tb = traces.synthetic_tables(name, loc)
            e.set_tables(loc, tb["W"], tb["C"], tb["T"], tb["WB"])
        for c, f in enumerate(("dc_config.json", "dc_config_r16.json")):
            e.set_dc_params(c, dc_config.size_datacenter(f, 1, 30.0))
        self.cfg = np.arange(N, dtype=np.int32) % 2
        self.loc = (np.arange(N, dtype=np.int32) // 2) % 2
        e.assign(self.loc, self.cfg, 174, 188)
        self.eng = e
        self.g = torch.Generator(device="cpu").manual_seed(3)

    def acts(self, k=None):
        shape = (N, 3) if k is None else (k, N, 3)
        return self.torch.randint(0, 3, shape, dtype=self.torch.int32, generator=self.g).cuda()

    def t_rel(self):
        return self.eng.get_state("t_rel")

    def check(self, what, t_want=None):
        """the host's copy == the device's arrays -> the device's t_rel"""
        e = self.eng
        t, cfg, loc = self.t_rel(), e.get_state("cfg_id"), e.get_state("loc_id")
        m = e.snapshot().manifest
        assert m[:, SNAP_T_REL].tolist() == t.tolist(), (what, "t_rel")
        assert m[:, SNAP_CFG_ID].tolist() == cfg.tolist() == self.cfg.tolist(), (what, "cfg_id")
        assert m[:, SNAP_LOC_ID].tolist() == loc.tolist() == self.loc.tolist(), (what, "loc_id")
        assert e.steps_to_episode_end() == EP - int(t.max()), (what, "steps_to_episode_end")
        if t_want is not None:
            assert t.tolist() == list(t_want), (what, "t_rel", t.tolist())
        return t

    def advance(self, what, k=None):
        """a step (k None) or a rollout of k steps, held to the kernel and the finished envs the device's t_rel before it predicts"""
        e = self.eng
        before = self.t_rel()
        path = "pair" if (before == before[0]).all() else "general"
        n = 1 if k is None else k
        assert n <= EP - int(before.max())
        if k is None:
            e.step(self.acts())
        else:
            e.rollout(self.acts(k))
        assert e.last_step_kernel() == (KERNEL_NAME if k is None else ROLLOUT_NAME)[path], (what, path)
        ended = before + n == EP
        done = e.last_done()
        assert (done is None and not ended.any()) or (done is not None and done.tolist() == ended.tolist()), (what, "last_done")
        after = np.where(ended, 0, before + n) if self.auto else before + n
        self.check(what, after)
        if not self.auto and ended.any():      # (what auto_reset would have done inside the call)
            e.reset(mask=ended.astype(np.uint8))
            self.check(what + ", the finished envs reset", np.where(ended, 0, before + n))

    def clone(self, src, dst):
        self.eng.clone_envs(src, dst)
        self.cfg[dst], self.loc[dst] = self.cfg[src], self.loc[src]


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_auto_reset"])
def test_host_copy_follows_the_device_across_entry_points(auto_reset):
    r = _Rig(auto_reset)
    e = r.eng
    e.reset()
    r.check("reset", [0] * N)
    for i in range(3):
        r.advance(f"step {i}")
    mask = np.zeros(N, dtype=np.uint8)
    mask[[1, 4, 6]] = 1
    e.reset(mask=mask)
    r.check("masked reset", [3, 0, 3, 3, 0, 3, 0, 3])
    r.advance("step out of lock-step")                                   # [4, 1, 4, 4, 1, 4, 1, 4]
    r.clone([0, 4], [1, 5])                                              # env 1 <- an env ahead of it, env 5 <- one behind it
    r.check("clone", [4, 4, 4, 4, 1, 1, 1, 4])
    snap = e.snapshot([0, 4])
    assert snap.manifest[:, SNAP_T_REL].tolist() == [4, 1]
    r.advance("step behind the snapshot")
    r.advance("step behind the snapshot")                                # [6, 6, 6, 6, 3, 3, 3, 6]
    e.restore(snap, envs=[2, 7], rows=[1, 0])                            # into other envs: they take the rows' config and location
    r.cfg[[2, 7]], r.loc[[2, 7]] = r.cfg[[4, 0]], r.loc[[4, 0]]
    r.check("restore", [6, 6, 1, 6, 3, 3, 3, 4])
    mk = e.mark(max_steps=4)
    r.advance("step behind the mark")
    r.advance("step behind the mark")
    e.rewind(mk)
    r.check("whole-batch rewind", [6, 6, 1, 6, 3, 3, 3, 4])
    mk = e.mark([0, 2], max_steps=2)
    r.advance("step behind the mark of two envs")
    e.rewind(mk)
    r.check("rewind of two envs", [6, 7, 1, 7, 4, 4, 4, 5])
    r.advance("rollout that ends the leaders' episode", k=e.steps_to_episode_end())      # 5 steps: envs 1 and 3 finish
    r.clone(np.full(N - 1, 2), np.delete(np.arange(N), 2))               # every env a copy of env 2: lock-step again
    r.check("clone of one env into all", [6] * N)
    r.advance("step in lock-step again")
    mk = e.mark(max_steps=3)
    r.advance("rollout behind the mark", k=3)
    e.rewind(mk)
    r.check("whole-batch rewind in lock-step", [7] * N)
    r.advance("step after the rewind")
    r.advance("rollout that ends every episode", k=e.steps_to_episode_end())
    r.advance("step of the new episodes")
    e.close()
