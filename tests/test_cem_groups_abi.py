"""sdc_plan_cem_groups on the CPU side: declared with its argument names, exported and bound with the ABI still at 313;
sdc_cem_group_params' ctypes mirror has the C compiler's size and offsets; the library refuses a null handle before it touches a
device; the translation unit cross-compiles for gfx950 with no scratch and no spills for exactly its two kernels, with the register,
LDS and occupancy figures DESIGN section 4.14 states; GroupCEMMPCAgent's host logic (the warm start's shift by a step, the
re-synchronisation and the fresh start when the episode step goes backwards) on CPU tensors, against an engine stub that records what
the agent asks of it."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from dc_rl_amd import _lib as L

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "sustaindc_hip.h")
ARGS = ["h", "n_steps", "cem", "objective", "probs", "best_seq", "best_score", "best_action", "step_actions", "cand", "cand_score", "obs",
        "share_obs", "stream"]
MEMBERS = ["group_size", "group_base", "n_iters", "iter0", "n_elite", "fixed_action", "draw", "seed", "alpha", "p_min"]
# DESIGN.md section 4.14's table: VGPRs, LDS bytes per workgroup, occupancy in wavefronts per SIMD
FIGURES = {"sdc_cem_group_sample_kernel": (36, 3552, 8), "sdc_cem_group_refit_kernel": (81, 9488, 5)}


def test_entry_point_is_declared_exported_and_bound_at_abi_313():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define SDC_ABI_VERSION 313\b", hdr)
    m = re.search(r"#define SDC_CEM_MAX_GROUP (\d+)", hdr)
    assert m and int(m.group(1)) == L.CEM_MAX_GROUP == 1024
    decl = re.search(r"\bint sdc_plan_cem_groups\(([^)]*)\);", hdr)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == ARGS, decl
    assert "sdc_plan_cem_groups" in L.EXPORTS
    assert L.ABI_VERSION == 313 and "sdc_cem_groups.hip" in L.SOURCES
    L.build()
    lib = C.CDLL(L.LIB_PATH)
    assert lib.sdc_version() == 313
    assert hasattr(lib, "sdc_plan_cem_groups")
    assert len(L.load().sdc_plan_cem_groups.argtypes) == len(ARGS)
    import dc_rl_amd
    from dc_rl_amd.agents import GroupCEMMPCAgent
    from dc_rl_amd.engine import GroupCEMResult, SdcEngine
    from dc_rl_amd.vec_env import SustainDCVecEnv
    assert dc_rl_amd.GroupCEMMPCAgent is GroupCEMMPCAgent and dc_rl_amd.GroupCEMResult is GroupCEMResult
    for cls in (SdcEngine, SustainDCVecEnv):
        assert callable(cls.plan_cem_groups) and callable(cls.sync_groups)
    from dc_rl_amd.multi_device import SustainDCMultiDeviceVecEnv
    assert not hasattr(SustainDCMultiDeviceVecEnv, "plan_cem_groups")


def test_params_mirror_has_the_c_layout(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(sdc_cem_group_params));']
    src += [f'  printf("{m} %zu\\n", offsetof(sdc_cem_group_params, {m}));' for m in MEMBERS]
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-o", exe, str(c)], check=True)
    out = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SdcCemGroupParams)
    for m in MEMBERS:
        assert int(out[m]) == getattr(L.SdcCemGroupParams, m).offset, m
    assert [f[0] for f in L.SdcCemGroupParams._fields_] == MEMBERS
    assert L.SdcCemGroupParams.fixed_action.size == 12 and L.SdcCemGroupParams.seed.size == 8 and L.SdcCemGroupParams.draw.size == 4


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_plan_cem_groups(None, 1, None, None, None, None, None, None, None, None, None, None, None, None) == -2
    assert b"sdc_plan_cem_groups: null handle" in lib.sdc_last_error()


def test_group_kernels_compile_for_gfx950_without_scratch_or_spills_at_the_documented_figures():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in L.HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc] + flags + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "sdc_cem_groups.hip",
                            "-o", os.path.join(td, "o.o")], cwd=L.CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    per, cur = {}, None
    for line in r.stderr.splitlines():
        f = re.search(r"remark:\s+Function Name: (\S+)", line)
        if f:
            cur = per.setdefault(f.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert set(per) == set(FIGURES), sorted(per)
    for k, u in per.items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert (u["VGPRs"], u["LDS Size"], u["Occupancy"]) == FIGURES[k], (k, u)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4.14"):]
    for k, (vgprs, lds, occ) in FIGURES.items():
        row = re.search(r"\| `%s` \| (\d+) \| ([\d ]+) \| (\d+) \|" % k, sec)
        assert row, k
        assert (int(row.group(1)), int(row.group(2).replace(" ", "")), int(row.group(3))) == (vgprs, lds, occ), (k, row.group(0))
    # the refit kernel's scores [1024] fp64 are 8 KiB of its LDS; a sample wavefront's LDS leaves the register file as the limit
    assert per["sdc_cem_group_refit_kernel"]["LDS Size"] >= 8 * L.CEM_MAX_GROUP
    assert 32 * per["sdc_cem_group_sample_kernel"]["LDS Size"] <= 160 * 1024


class _Stub:
    """What GroupCEMMPCAgent.act asks of an engine, on the CPU: sync_groups and plan_cem_groups record their arguments; the latter
    answers with tensors that tell the step and the decision apart (best_seq[k] = 100 d + 10 k + agent, probs[k] = d + k / 16 +
    (agent, action) / 256, step_actions = best_seq[0] of the env's group)."""

    def __init__(self, n_envs=6, episode_steps=12):
        import torch
        self.n_envs, self.device = n_envs, torch.device("cpu")
        self.config = dict(auto_reset=True, episode_steps=episode_steps)
        self.t, self.calls, self.syncs = 0, [], []

    def steps_to_episode_end(self):
        return self.config["episode_steps"] - self.t

    def step(self):
        self.t = (self.t + 1) % self.config["episode_steps"]

    def sync_groups(self, R):
        self.syncs.append((len(self.calls), R))

    def plan_cem_groups(self, R, K, n_iters, E, *, probs, best_seq, draw, **kw):
        import torch
        from dc_rl_amd.engine import GroupCEMResult
        self.calls.append(dict(R=R, K=K, probs=None if probs is None else probs.clone(), best_seq=None if best_seq is None else best_seq.clone(),
                               draw=draw, n_iters=n_iters, E=E, **kw))
        d, G = len(self.calls), self.n_envs // R
        k = torch.arange(K).view(K, 1, 1)
        seq = (100 * d + 10 * k + torch.arange(3).view(1, 1, 3)).expand(K, G, 3).to(torch.int32).contiguous()
        p = (d + k.view(K, 1, 1, 1) / 16.0 + torch.arange(9).view(1, 1, 3, 3) / 256.0).expand(K, G, 3, 3).to(torch.float64).contiguous()
        return GroupCEMResult(seq[0].clone(), seq[0].repeat_interleave(R, dim=0), seq, torch.zeros((n_iters, G), dtype=torch.float64), p,
                              None, None)


def test_agent_warm_start_shifts_by_a_step_and_resyncs_and_starts_afresh_when_the_episode_step_goes_backwards():
    import pytest
    import torch
    from dc_rl_amd.agents import GroupCEMMPCAgent
    R, G = 3, 2
    e = _Stub(n_envs=R * G, episode_steps=12)
    ag = GroupCEMMPCAgent(R, n_elite=2, n_iters=3, horizon=4, seed=9, alpha=0.25, p_min=0.01)
    third = 1.0 / 3.0
    nothing = torch.tensor([1, 1, 2], dtype=torch.int32)

    def expect_seq(d, K):      # decision d's result moved up by a step: steps 1 .. K-1 of it, then do-nothing; per GROUP
        rows = [[[100 * d + 10 * k + a for a in range(3)]] * G for k in range(1, K)] + [[[1, 1, 2]] * G]
        return torch.tensor(rows, dtype=torch.int32)

    def expect_probs(d, K):
        rows = [[[[d + k / 16.0 + (3 * a + j) / 256.0 for j in range(3)] for a in range(3)]] * G for k in range(1, K)]
        rows += [[[[third] * 3] * 3] * G]
        return torch.tensor(rows, dtype=torch.float64)

    # decision 1: the groups are synchronised first, nothing to start from; the action is every replica's
    a = ag.act(e)
    assert e.syncs == [(0, R)] and ag.syncs == 1
    assert a.shape == (R * G, 3) and torch.equal(a, torch.tensor([[100, 101, 102]] * (R * G), dtype=torch.int32))
    c = e.calls[-1]
    assert c["probs"] is None and c["best_seq"] is None and c["draw"] == 0 and c["K"] == 4 and c["R"] == R
    assert (c["n_iters"], c["E"], c["seed"], c["alpha"], c["p_min"]) == (3, 2, 9, 0.25, 0.01)
    # decisions 2 and 3: the one before, shifted; no further synchronisation inside the episode
    for d in (1, 2):
        e.step()
        ag.act(e)
        c = e.calls[-1]
        assert c["draw"] == d and c["K"] == 4
        assert c["best_seq"].dtype == torch.int32 and torch.equal(c["best_seq"], expect_seq(d, 4)), d
        assert c["probs"].dtype == torch.float64 and torch.equal(c["probs"], expect_probs(d, 4)), d
    assert len(e.syncs) == 1
    # towards the episode's end the horizon shrinks and the shift follows it
    while e.steps_to_episode_end() > 4:
        e.step()
        ag.act(e)
    assert e.calls[-1]["K"] == 3 and ag.last_horizon == 3
    d = len(e.calls)
    assert torch.equal(e.calls[-1]["best_seq"], expect_seq(d - 1, 3)) and torch.equal(e.calls[-1]["probs"], expect_probs(d - 1, 3))
    e.step()
    ag.act(e)
    e.step()
    ag.act(e)
    assert e.calls[-1]["K"] == 1 and torch.equal(e.calls[-1]["best_seq"], nothing.expand(1, G, 3))
    # one step left: no plan, every replica does nothing
    e.step()
    n = len(e.calls)
    assert e.steps_to_episode_end() == 1
    assert torch.equal(ag.act(e), nothing.expand(R * G, 3)) and len(e.calls) == n and ag.last is None and ag.last_horizon == 0
    assert len(e.syncs) == 1
    # the episode step goes backwards: the groups are synchronised again BEFORE the plan, both start afresh, the counter goes on
    e.step()
    assert e.steps_to_episode_end() == 12
    ag.act(e)
    c = e.calls[-1]
    assert e.syncs == [(0, R), (n, R)] and ag.syncs == 2
    assert c["probs"] is None and c["best_seq"] is None and c["draw"] == n and c["K"] == 4
    e.step()
    ag.act(e)
    assert torch.equal(e.calls[-1]["best_seq"], expect_seq(n + 1, 4)) and len(e.syncs) == 2
    e.step()
    ag.act(e)
    e.t = 0      # ... also straight from a warm decision
    ag.act(e)
    assert e.calls[-1]["probs"] is None and e.calls[-1]["best_seq"] is None and len(e.syncs) == 3 and e.syncs[-1] == (len(e.calls) - 1, R)
    with pytest.raises(ValueError, match="group_size"):
        GroupCEMMPCAgent(1)
    with pytest.raises(ValueError, match="n_elite"):
        GroupCEMMPCAgent(4, n_elite=5)
