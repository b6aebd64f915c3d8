"""Parity in the PRODUCTION configuration at the sizes and kernels the bench line quotes rates for.

One recipe, shared by tests/test_gpu_timed_config.py, tests/test_gpu_production_sizes.py, tests/test_gpu_throughput_regime.py and
tests/test_gpu_kernel_reach.py: `debug_flags` as given (0 = what bench.py times: no verify kernel), auto-reset with the device's own
Philox resets, every history ring at its 10 000-entry steady state (write positions spread, duplicates included), i.i.d. uniform
actions, deferred window re-centring by the spare wavefronts under the full request load -- and a SAMPLE of envs, chosen from the
geometry of the step kernel under test (`sample_envs`), stepped by the fp64 oracle on the device's own episode windows (read back
after every reset, and held to the NumPy restatement of the device's draw scheme: `ProductionRig.begin_all`).
Reference: sustaindc_env.py:533-621 (step), utils/reward_creator.py:16-45 (normalize_energy)."""
from dataclasses import dataclass

import numpy as np

from dc_rl_amd import _lib as L
from dc_rl_amd import dc_config, traces
from dc_rl_amd.engine import SdcEngine
from oracle import pyoracle as po
from tests import gpu_helpers as G
from tests import reset_ref as RR
from tests.parity_util import INFO_CMP

TOL = 1e-5   # north_star: 1e-5 relative fp32 (absolute where |ref| < 1)
DRAW_TOL = 2e-6   # C: the device's fp32 transcendentals against NumPy's (tests/test_gpu_reset_pin.py)
CAP = 10000
MIXED_FILES = ("dc_config.json", "dc_config_r16.json", "dc_config_r25.json")
MIXED_LOCATIONS = ("ny", "az", "wa")
RING_CHUNK = 8192      # envs per block of the ring injection (a [8192, 10000] fp32 block: 328 MB)

# MI355X: 256 CUs, 4 SIMDs per CU, 160 KiB of LDS per CU (csrc/sdc_tuning.hpp SDC_CUS)
CUS, SIMDS_PER_CU, LDS_PER_CU = 256, 4, 160 * 1024


@dataclass(frozen=True)
class KernelGeometry:
    """How a step kernel's grid covers the envs: `envs_per_wg` envs per env workgroup, `envs_per_wave` per env wavefront
    (the lane-per-env kernel: both wavefronts of a workgroup serve the same 64 envs), `waves_per_wg` wavefronts per workgroup,
    `wgs_per_cu` workgroups resident per CU -- the smaller of what the VGPRs allow (waves per SIMD, the compiler's occupancy)
    and what the LDS allows.  tests/test_isa_guard.py::test_sampler_residency_matches_the_compiled_kernels derives it from the
    compiled code and holds this table to it."""
    kernel: str
    envs_per_wave: int
    waves_per_wg: int
    envs_per_wg: int
    wgs_per_cu: int
    sweeps: str            # the spare (re-centring) workgroups FIRST in the grid: "coop", "wide" or "none"

    def env_blocks(self, N):
        return -(-N // self.envs_per_wg)     # csrc/sdc_dispatch.hpp sdc_env_blocks

    def sweep_blocks(self, N):
        """sdc_capi.hip: d.sweep_blocks (sdc_create) for the pair / quad / general kernels, launch_step's for the lane-per-env
        kernel (half the request capacity d.rq_max, at most 128), none in the multi-step kernels."""
        if self.sweeps == "coop":
            return min(128, max(32, N // 128))
        if self.sweeps == "wide":
            rq_max = min(2047, max(128, (N // 32 + 127) // 128 * 128))     # SDC_RQ_LIMIT, SDC_RQ_MIN
            return min(rq_max, 256) // 2
        return 0


# (residency: SDC_STEP_WAVES_PER_EU / SDC_QUAD_WAVES_PER_EU = 3 wavefronts per SIMD -> 12 per CU = three 4-wavefront workgroups;
# the lane-per-env kernel two per SIMD (233 VGPRs) -> four 2-wavefront workgroups, its LDS 40 KB -> four; the general form's
# 51.4 KB of LDS -> three: DESIGN.md section 4.3)
GEOMETRY = {
    "general": KernelGeometry("sdc_dynamics_kernel", 2, 4, 8, 3, "coop"),
    "pair": KernelGeometry("sdc_dynamics_fast_kernel", 2, 4, 8, 3, "coop"),
    "quad": KernelGeometry("sdc_dynamics_quad_kernel", 4, 4, 16, 3, "coop"),
    "wide": KernelGeometry("sdc_dynamics_wide_kernel", 64, 2, 64, 4, "wide"),
    "wide_gen": KernelGeometry("sdc_dynamics_wide_gen_kernel", 64, 2, 64, 3, "wide"),
}


def env_block_of_workgroup(b, n_blocks):
    """csrc/sdc_sweep.hpp first_pair_of_block (divided by its `wpb`): env workgroup b (after the sweep workgroups) -> the env
    block it steps.  Every XCD (workgroup b runs on XCD b % 8) a contiguous range when the count divides by 8, else the identity."""
    return (b % 8) * (n_blocks // 8) + b // 8 if n_blocks % 8 == 0 else b


def sample_parts(N, geom):
    """The deterministic part of the sample, by reason: {"first": [...], "last": [...], "rounds": {b: [...]}} -- every env of
    the first and the last env workgroup (the first / last env wavefronts, the ragged last workgroup), and of the env workgroups
    either side of every occupancy round boundary: a round holds CUS * wgs_per_cu workgroups of the grid, the sweep workgroups
    first -- boundaries at dispatch position k * cap, i.e. env workgroup k * cap - sweeps, and at env workgroup k * cap (the
    sweeps retire early and hand their slots on); and "cu_steps": either side of every CUS-th env workgroup, where the dispatcher
    starts another workgroup on every CU and the pair / quad kernels switch the issue priority (sdc_sweep.hpp set_round_priority).
    Boundary workgroups of four or more wavefronts are sampled at the first and last env of every wavefront, the lane-per-env
    kernel's at lanes 0, 1, 31, 32, 62, 63."""
    nb, sw = geom.env_blocks(N), geom.sweep_blocks(N)
    cap = CUS * geom.wgs_per_cu

    def envs_of(b, every):
        e0 = env_block_of_workgroup(b, nb) * geom.envs_per_wg
        if every:
            picks = range(geom.envs_per_wg)
        elif geom.envs_per_wave == geom.envs_per_wg:
            picks = (0, 1, 31, 32, 62, 63)
        else:
            picks = [w * geom.envs_per_wave + j for w in range(geom.envs_per_wg // geom.envs_per_wave)
                     for j in (0, geom.envs_per_wave - 1)]
        return sorted({e0 + j for j in picks if e0 + j < N})

    rounds = {}
    k = 1
    while k * cap < sw + nb:
        for b0 in (k * cap - sw, k * cap):
            for b in (b0 - 1, b0):
                if 0 <= b < nb:
                    rounds[b] = envs_of(b, geom.envs_per_wg <= 8)
        k += 1
    cu_steps = {b: envs_of(b, geom.envs_per_wg <= 8) for m in range(CUS, nb, CUS) for b in (m - 1, m)}
    return dict(first=envs_of(0, True), last=envs_of(nb - 1, True), rounds=rounds, cu_steps=cu_steps)


def sample_envs(N, geom, rng, n_random=56):
    """Envs to check for a batch of N on the kernel of `geom`: `sample_parts` plus a random spread of n_random envs."""
    p = sample_parts(N, geom)
    s = set(p["first"]) | set(p["last"])
    for v in list(p["rounds"].values()) + list(p["cu_steps"].values()):
        s |= set(v)
    if n_random:
        s |= set(int(x) for x in rng.choice(N, min(n_random, N), replace=False))
    return sorted(s)


def fill_rings(hist, seed, cap=CAP, chunk=RING_CHUNK):
    """Every ring of hist [N, stride] (fp32, the buffer that goes to set_state) at its steady state, generated block by block on
    the device (a seeded generator: the same rings for the same seed) into that buffer: keys ~ 331 +- 70 clipped to [150, 650],
    every 97th slot a duplicate of slot 5; the slots behind `cap` empty (NaN)."""
    import torch
    N = hist.shape[0]
    hist[:, cap:] = np.nan
    g = torch.Generator(device="cuda").manual_seed(seed)
    for lo in range(0, N, chunk):
        v = torch.randn((min(chunk, N - lo), cap), generator=g, device="cuda", dtype=torch.float32)
        v = (v * 70 + 331).clamp_(150, 650)
        v[:, ::97] = v[:, 5:6]
        hist[lo:lo + chunk, :cap] = v.cpu().numpy()


class ProductionRig:
    """N envs on one engine in the production configuration + oracles for a sample of them.  `mapping` names the step kernel
    the sample is built for (GEOMETRY); the first single step asserts that the engine did launch it."""

    def __init__(self, N, mapping, debug_flags=0, mixed=False, episode_steps=120, seed=77, n_random=56,
                 reward_method=(0, 0, 0), policy=(0, 0, 0), trim_and_respond_limit=27.0, env_index_base=0, dc_files=None,
                 oracles=True, hist_cap=CAP, sample=None, queue_max_len=None, day_range=None):
        """sample: the envs to hold to the oracle, instead of the geometry's (`sample_envs`); queue_max_len: the engine's and the
        oracles' (None: their default, 1000); day_range: (first, last) start day of every env (None: the fortnight around 1 July)."""
        self.N, self.steps, self.seed, self.env_index_base = N, episode_steps, seed, env_index_base
        self.geom = GEOMETRY[mapping]
        self.cap = hist_cap
        assert hist_cap == CAP or not oracles, "the oracle's ring holds CAP keys"
        rng = self.rng = np.random.default_rng(seed)
        locs = MIXED_LOCATIONS if mixed else ("ny",)
        files = dc_files if dc_files is not None else (MIXED_FILES if mixed else ("dc_config.json",))
        self.tables = [traces.synthetic_tables(loc, 0) for loc in locs]
        combos = [(li, f) for li in range(len(locs)) for f in files]
        self.params = [dc_config.size_datacenter(f, 1, traces.max_ambient_for_sizing(traces.obtain_paths(locs[li])[0]))
                       for li, f in combos]
        # (kept: restore() builds a second engine exactly like this one)
        self.engine_kw = dict(episode_steps=episode_steps, auto_reset=True, seed=seed, debug_flags=debug_flags,
                              n_locations=len(locs), n_dc_configs=len(combos), reward_method=reward_method, policy=policy,
                              trim_and_respond_limit=trim_and_respond_limit, env_index_base=env_index_base, hist_cap=hist_cap)
        if queue_max_len is not None:
            self.engine_kw["queue_max_len"] = queue_max_len
        e = np.arange(N)
        # BASELINE configs[3]: the rack count follows env_id % 3; the location changes every three envs
        self.loc_id = ((e // len(files)) % len(locs)).astype(np.int32)
        self.cfg_id = (self.loc_id * len(files) + e % len(files)).astype(np.int32)
        init_day = traces.get_init_day(6)
        self.day_lo, self.day_hi = (init_day - 7, init_day + 7) if day_range is None else day_range
        eng = self.eng = self.make_engine()
        self.sample = sample_envs(N, self.geom, rng, n_random) if sample is None else sorted(int(i) for i in sample)
        # steady-state history: every ring full, write positions spread, duplicates included -- generated in place in the buffer
        # set_state hands to the library (no second host copy); only the sampled envs' rings are kept, for their oracles
        hist = np.empty((N, eng.hist_stride), np.float32)
        fill_rings(hist, seed, hist_cap)
        pos = rng.integers(0, hist_cap, N).astype(np.int32)
        vals = {i: hist[i, :CAP].astype(np.float64) for i in self.sample} if oracles else {}
        eng.set_state("hist", hist)
        del hist
        eng.set_state("hist_len", np.full(N, hist_cap, np.int32))
        eng.set_state("hist_pos", pos)
        self.orcs = {}
        for i in vals:
            p = dict(self.params[self.cfg_id[i]], reward_method=tuple(int(m) for m in reward_method))
            if queue_max_len is not None:
                p["queue_max_len"] = queue_max_len
            o = po.OracleEnv(G.oracle_params_from_dict(p))
            o.e.stpt = float(p["init_setpoint"])
            o.e.hist_len = CAP
            o.e.hist_pos = int(pos[i])
            np.ctypeslib.as_array(o.e.hist)[:] = vals[i]
            self.orcs[i] = o
        del vals
        self.worst = dict(obs=0.0, rew=0.0, info=0.0, draw=0.0)
        self.paths = np.zeros(8, np.int64)
        self.resets = 0
        self.draws_checked = 0
        self.kernel_checked = False
        self._idx = None
        self.twin = None          # restore(keep_twin=True): the engine the checkpoint came from, stepped alongside
        self.restored = None      # after restore(): "general" until the restored engine's first episode boundary, then "specialised"
        self.restore_kernels = {"general": set(), "specialised": set()}
        self.twin_kernels = set()

    def make_engine(self, cfg_id=None, **overrides):
        """A fresh engine with this rig's constructor arguments, tables, DC parameters and assignment (cfg_id: another
        assignment of the DC configs) -- and empty rings: nothing is injected."""
        eng = SdcEngine(self.N, **dict(self.engine_kw, **overrides))
        for li, tb in enumerate(self.tables):
            eng.set_tables(li, tb["W"], tb["C"], tb["T"], tb["WB"])
        for ci, p in enumerate(self.params):
            eng.set_dc_params(ci, p)
        eng.assign(self.loc_id, self.cfg_id if cfg_id is None else cfg_id, self.day_lo, self.day_hi)
        return eng

    def restore(self, keep_twin=True, cfg_id=None, **overrides):
        """Checkpoint the engine (state_dict), load the checkpoint into a fresh engine (make_engine, then reset(), then
        load_state_dict) and go on with that one: the oracles are not touched, so they hold the restored engine ("B") to the same
        trajectory -- including begin_all's check of its next reset draws, which are keyed on the seed, env_index_base and the
        episode counter the checkpoint carries.  keep_twin: the old engine ("A") stays as `twin`; step() steps it alongside and
        holds every env of B to it bit for bit.  A restored engine has no feature rows: step() asserts that it runs
        sdc_dynamics_kernel until its first episode boundary and the kernel of the sample's mapping after it.  -> the checkpoint."""
        sd = self.eng.state_dict()
        b = self.make_engine(cfg_id=cfg_id, **overrides)
        b.reset()
        b.load_state_dict(sd)
        if keep_twin:
            self.twin = self.eng
        else:
            self.eng.close()
        self.eng = b
        self.restored = "general"
        return sd

    def check_draws(self, st, tw, wb):
        """The device's own reset of every sampled env against tests/reset_ref.py (its Philox draw scheme restated): day, hour,
        cursor and the carbon-intensity bounds exactly, the weather windows and bounds within DRAW_TOL -- keyed on the engine's
        seed, the env's GLOBAL index (env_index_base + i), the episode number the device holds and the env's day range."""
        ep = self.eng.get_state("episode")
        for i in self.orcs:
            x = RR.device_reset_expected(self.tables[self.loc_id[i]], self.seed, self.env_index_base + i, int(ep[i]),
                                         self.day_lo, self.day_hi, self.steps)
            got = (int(st["day"][i]), int(st["hourq"][i]) // 4, int(st["cursor"][i]))
            assert got == (x["day"], x["hour"], x["c0"]), (i, int(ep[i]), got, (x["day"], x["hour"], x["c0"]))
            assert st["ci_min"][i] == x["ci_min"] and st["ci_den"][i] == x["ci_den"], (i, int(ep[i]))
            e = max(np.abs(tw[i] - x["t_win"]).max(), np.abs(wb[i] - x["wb_win"]).max(), abs(st["t_min"][i] - x["t_min"]),
                    abs(st["t_den"][i] - x["t_den"]))
            assert e <= DRAW_TOL, (i, int(ep[i]), float(e))
            self.worst["draw"] = max(self.worst["draw"], float(e))
            self.draws_checked += 1

    def begin_all(self, obs_dev, check_draws=True):
        """Start the oracles' next episode on the windows the DEVICE drew (read back; first held to the draw scheme:
        check_draws); compares the reset observations."""
        eng, steps = self.eng, self.steps
        raw = G.raw_obs(obs_dev[self.sample_index()].cpu().numpy())
        st = {k: eng.get_state(k) for k in ("cursor", "day", "hourq", "t_min", "t_den", "ci_min", "ci_den")}
        tw, wb = eng.get_state("t_win"), eng.get_state("wb_win")
        if check_draws:
            self.check_draws(st, tw, wb)
        for j, i in enumerate(self.sample):
            o = self.orcs.get(i)
            if o is None:
                continue
            tb = self.tables[self.loc_id[i]]
            c0 = int(st["cursor"][i])
            lo, hi = max(0, c0 - 16), c0 + steps + 18
            T = np.zeros(hi - lo)
            WBv = np.zeros(hi - lo)
            T[c0 - lo:] = tw[i]
            WBv[c0 - lo:] = wb[i]
            NC = (tb["C"][lo:hi] - st["ci_min"][i]) / st["ci_den"][i]
            NT = (T - st["t_min"][i]) / st["t_den"][i]
            oo = o.begin(tb["W"][lo:hi], tb["C"][lo:hi], NC, T, WBv, NT, lo, int(st["day"][i]), int(st["hourq"][i]) // 4, steps)
            self.worst["obs"] = max(self.worst["obs"], float(G.rel_err(raw[j], oo).max()))

    def sample_index(self):
        import torch
        if self._idx is None:
            self._idx = torch.tensor(self.sample, dtype=torch.int64, device=self.eng.device)
        return self._idx

    def check_step(self, a_s, eo, er, ed, ei, fo):
        """One step's outputs of the SAMPLED envs (host arrays, row j = env sample[j]; eo / fo raw [S, 53]; ei None: a step
        without the info rows) against the oracle under their actions a_s [S, 3]."""
        w = self.worst
        cols = [po.INFO_IDX[k] for k in INFO_CMP]     # same column order in product and oracle for the first 37 columns
        for j, i in enumerate(self.sample):
            o = self.orcs.get(i)
            if o is None:
                continue
            oo, orew, odone, oinfo = o.step(a_s[j])
            assert int(ed[j]) == odone
            # at an episode end the step's own observation is in final_obs; obs already holds the next episode's first
            w["obs"] = max(w["obs"], float(G.rel_err(fo[j] if odone else eo[j], oo).max()))
            w["rew"] = max(w["rew"], float(G.rel_err(er[j], orew).max()))
            if ei is not None:
                w["info"] = max(w["info"], float(G.rel_err(ei[j, cols], np.asarray(oinfo)[cols]).max()))

    def _device_checks(self, info, done):
        """Whole-batch checks reduced on the device: no fault anywhere, the reward-state path histogram (info None: a step
        without the info rows); -> number of envs done."""
        import torch
        if info is not None:
            assert not bool((info[..., L.INFO_IDX["fault"]] != 0).any())
            self.paths += torch.bincount(info[..., L.INFO_IDX["reserved"]].reshape(-1).to(torch.int64), minlength=8)[:8].cpu().numpy()
        return int(done.sum())

    def check_kernel(self):
        got = self.eng.last_step_kernel()
        assert got == self.geom.kernel, f"the sample was built for {self.geom.kernel}, the step ran {got}"
        self.kernel_checked = True

    def check_restored_kernel(self, kernel, done):
        """After restore(): the kernel the restored engine ran for the launch that has just ended (done: it ended an episode)."""
        self.restore_kernels[self.restored].add(kernel)
        want = "sdc_dynamics_kernel" if self.restored == "general" else self.geom.kernel
        assert kernel == want, f"restored engine, {self.restored} phase: expected {want}, ran {kernel}"
        if done:
            self.restored = "specialised"

    def twin_equal(self, a_out, b_out, what, final_obs=False):
        """Every env of the restored engine's outputs (obs, share_obs, rew, done, info[, ...]) against the twin's, bit for bit -- the
        info diagnostics column aside (it says HOW the reward state was served, which a restore changes); final_obs: also the
        engines' final_obs buffers."""
        import torch
        names = ("obs", "share_obs", "rew", "done", "info")
        pairs = list(zip(names, a_out[:5], b_out[:5]))
        if final_obs:
            pairs.append(("final_obs", self.twin.final_obs, self.eng.final_obs))
        for nm, u, v in pairs:
            if u is None and v is None:
                continue
            if nm == "info":
                u, v = u.clone(), v.clone()
                u[..., L.INFO_IDX["reserved"]] = 0
                v[..., L.INFO_IDX["reserved"]] = 0
            if not torch.equal(u, v):
                bad = (u != v).nonzero()
                raise AssertionError((what, nm, bad[:6].tolist(), u[tuple(bad[0])].item(), v[tuple(bad[0])].item()))

    def step(self, a_dev, want_info=True):
        """One single step under actions a_dev (int32 [N, 3] on the device), the sampled envs against the oracle, the auto-reset
        followed; -> the engine's (obs, share_obs, rew, done, info) views (want_info False: a step without the info rows, which
        is never one of the specialised kernels: csrc/sdc_dispatch.hpp sdc_specialised_ok)."""
        eng, idx = self.eng, self.sample_index()
        out = eng.step(a_dev, want_info=want_info)
        if self.restored is None and not self.kernel_checked:
            self.check_kernel()
        obs, share, rew, done, info = out
        info = info if want_info else None
        n_done = self._device_checks(info, done)
        assert n_done in (0, self.N), n_done
        if self.restored is not None:
            self.check_restored_kernel(eng.last_step_kernel(), n_done > 0)
        if self.twin is not None:
            a_out = self.twin.step(a_dev, want_info=want_info)
            self.twin_kernels.add(self.twin.last_step_kernel())
            self.twin_equal(a_out, out, "single step", final_obs=n_done > 0)
        fo = G.raw_obs(eng.final_obs[idx].cpu().numpy()) if n_done else None
        self.check_step(a_dev[idx].cpu().numpy(), G.raw_obs(obs[idx].cpu().numpy()), rew[idx].cpu().numpy(),
                        done[idx].cpu().numpy(), None if info is None else info[idx].cpu().numpy(), fo)
        if n_done:
            self.resets += 1
            self.begin_all(obs)
        return out

    def single_steps(self, n_steps, seed=78):
        import torch
        arng = torch.Generator(device="cpu").manual_seed(seed)
        for t in range(n_steps):
            self.step(torch.randint(0, 3, (self.N, 3), dtype=torch.int32, generator=arng).cuda())

    def check_rollout(self, acts, out):
        """The K steps of a multi-step launch (obs [K,N,3,26], share, rew, done, info, ...) under actions acts [K,N,3]."""
        idx = self.sample_index()
        obs, rew, done, info = out[0], out[2], out[3], out[4]
        K = obs.shape[0]
        for k in range(K):
            n_done = self._device_checks(info[k], done[k])
            assert n_done in (0, self.N) and (n_done == 0 or k == K - 1), (k, n_done)
        a = acts[:, idx.to(acts.device)].cpu().numpy()
        so, sr, sd, si = (x[:, idx].cpu().numpy() for x in (obs, rew, done, info))
        fo = G.raw_obs(self.eng.final_obs[idx].cpu().numpy()) if sd[-1].any() else None
        for k in range(K):
            self.check_step(a[k], G.raw_obs(so[k]), sr[k], sd[k], si[k], fo if k == K - 1 else None)

    def assert_ok(self):
        w = self.worst
        assert w["obs"] <= TOL and w["rew"] <= TOL and w["info"] <= TOL, w
        assert (self.eng.get_state("hist_len") == self.cap).all()
        assert self.draws_checked >= len(self.orcs), (self.draws_checked, len(self.orcs))

    def assert_all_reward_state_paths_seen(self):
        """The three ways a step's reward state is served all occurred: without a ring read, by taking over a deferred
        re-centred window, and with the ring read inside the step (rebuild after the injection / inline re-centring)."""
        p = self.paths
        assert p[0] > 0 and p[2] > 0 and p[1] + p[3] > 0, p
        assert p[0] + p[2] > 50 * (p[1] + p[3] - self.N), p   # (one rebuild per env right after the injection)
