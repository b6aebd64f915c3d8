"""sdc_plan_cem on the CPU side: declared with its argument names, exported and bound with the ABI still at 313; sdc_cem_params' ctypes
mirror has the C compiler's size and offsets; the library refuses a null handle before it touches a device; the translation unit
cross-compiles for gfx950 with no scratch, no spills and an occupancy of at least 4 for exactly its two kernels; CEMMPCAgent's warm
start (the shift of best_seq and probs by a step, the fresh start when the episode step goes backwards) on CPU tensors, against an
engine stub that records what the agent hands to plan_cem."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from dc_rl_amd import _lib as L

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "sustaindc_hip.h")
ARGS = ["h", "n_steps", "cem", "objective", "probs", "best_seq", "best_score", "best_action", "cand", "cand_score", "obs", "share_obs",
        "stream"]
MEMBERS = ["n_iters", "iter0", "n_cand", "n_elite", "fixed_action", "draw", "seed", "alpha", "p_min"]


def test_cem_entry_point_is_declared_exported_and_bound_at_abi_313():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define SDC_ABI_VERSION 313\b", hdr)
    m = re.search(r"#define SDC_CEM_MAX_CAND (\d+)", hdr)
    assert m and int(m.group(1)) == L.CEM_MAX_CAND == 64
    decl = re.search(r"\bint sdc_plan_cem\(([^)]*)\);", hdr)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == ARGS, decl
    assert "sdc_plan_cem" in L.EXPORTS
    assert L.ABI_VERSION == 313 and "sdc_cem.hip" in L.SOURCES
    L.build()
    lib = C.CDLL(L.LIB_PATH)
    assert lib.sdc_version() == 313
    assert hasattr(lib, "sdc_plan_cem")
    assert len(L.load().sdc_plan_cem.argtypes) == len(ARGS)
    import dc_rl_amd
    from dc_rl_amd.agents import CEMMPCAgent
    from dc_rl_amd.engine import CEMResult
    assert dc_rl_amd.CEMMPCAgent is CEMMPCAgent and dc_rl_amd.CEMResult is CEMResult


def test_params_mirror_has_the_c_layout(tmp_path):
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
           '  printf("sizeof %zu\\n", sizeof(sdc_cem_params));']
    src += [f'  printf("{m} %zu\\n", offsetof(sdc_cem_params, {m}));' for m in MEMBERS]
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-o", exe, str(c)], check=True)
    out = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.SdcCemParams)
    for m in MEMBERS:
        assert int(out[m]) == getattr(L.SdcCemParams, m).offset, m
    assert [f[0] for f in L.SdcCemParams._fields_] == MEMBERS
    assert L.SdcCemParams.fixed_action.size == 12 and L.SdcCemParams.seed.size == 8 and L.SdcCemParams.draw.size == 4


def test_null_handle_is_refused_before_any_device_work():
    lib = L.load()
    assert lib.sdc_plan_cem(None, 1, None, None, None, None, None, None, None, None, None, None, None) == -2
    assert b"sdc_plan_cem: null handle" in lib.sdc_last_error()


def test_cem_kernels_compile_for_gfx950_without_scratch_or_spills():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in L.HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc] + flags + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "sdc_cem.hip",
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
    assert set(per) == {"sdc_cem_sample_kernel", "sdc_cem_refit_kernel"}, sorted(per)
    for k, u in per.items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert u["Occupancy"] >= 4, (k, u)
    # the refit kernel's LDS: four workgroups of four wavefronts fit a CU's 160 KiB, as its header says
    assert 4 * per["sdc_cem_refit_kernel"]["LDS Size"] <= 160 * 1024, per["sdc_cem_refit_kernel"]


class _Stub:
    """What CEMMPCAgent.act asks of an engine, on the CPU: plan_cem records its arguments and answers with tensors that tell the step
    and the decision apart (best_seq[k] = 100 d + 10 k + agent, probs[k] = d + k / 16 + (agent, action) / 256)."""

    def __init__(self, n_envs=2, episode_steps=12):
        import torch
        self.n_envs, self.device = n_envs, torch.device("cpu")
        self.config = dict(auto_reset=True, episode_steps=episode_steps)
        self.t, self.calls = 0, []

    def steps_to_episode_end(self):
        return self.config["episode_steps"] - self.t

    def step(self):
        self.t = (self.t + 1) % self.config["episode_steps"]

    def plan_cem(self, K, n_iters, M, E, *, probs, best_seq, draw, **kw):
        import torch
        from dc_rl_amd.engine import CEMResult
        self.calls.append(dict(K=K, probs=None if probs is None else probs.clone(), best_seq=None if best_seq is None else best_seq.clone(),
                               draw=draw, n_iters=n_iters, M=M, E=E, **kw))
        d, N = len(self.calls), self.n_envs
        k = torch.arange(K).view(K, 1, 1)
        seq = (100 * d + 10 * k + torch.arange(3).view(1, 1, 3)).expand(K, N, 3).to(torch.int32).contiguous()
        p = (d + k.view(K, 1, 1, 1) / 16.0 + torch.arange(9).view(1, 1, 3, 3) / 256.0).expand(K, N, 3, 3).to(torch.float64).contiguous()
        return CEMResult(seq[0].clone(), seq, torch.zeros((n_iters, N), dtype=torch.float64), p, None, None)


def test_warm_start_shifts_by_a_step_and_starts_afresh_when_the_episode_step_goes_backwards():
    import torch
    from dc_rl_amd.agents import CEMMPCAgent
    e = _Stub(n_envs=2, episode_steps=12)
    ag = CEMMPCAgent(n_candidates=6, n_elite=2, n_iters=3, horizon=4, seed=9, alpha=0.25, p_min=0.01)
    third = 1.0 / 3.0
    nothing = torch.tensor([1, 1, 2], dtype=torch.int32)

    def expect_seq(d, K):      # decision d's result moved up by a step: steps 1 .. K-1 of it, then do-nothing
        rows = [[[100 * d + 10 * k + a for a in range(3)]] * 2 for k in range(1, K)] + [[[1, 1, 2]] * 2]
        return torch.tensor(rows, dtype=torch.int32)

    def expect_probs(d, K):
        rows = [[[[d + k / 16.0 + (3 * a + j) / 256.0 for j in range(3)] for a in range(3)]] * 2 for k in range(1, K)]
        rows += [[[[third] * 3] * 3] * 2]
        return torch.tensor(rows, dtype=torch.float64)

    # decision 1: nothing to start from; decisions 2 and 3: the one before, shifted
    a = ag.act(e)
    assert torch.equal(a, torch.tensor([[100, 101, 102]] * 2, dtype=torch.int32))
    c = e.calls[-1]
    assert c["probs"] is None and c["best_seq"] is None and c["draw"] == 0 and c["K"] == 4
    assert (c["n_iters"], c["M"], c["E"], c["seed"], c["alpha"], c["p_min"]) == (3, 6, 2, 9, 0.25, 0.01)
    for d in (1, 2):
        e.step()
        ag.act(e)
        c = e.calls[-1]
        assert c["draw"] == d and c["K"] == 4
        assert c["best_seq"].dtype == torch.int32 and torch.equal(c["best_seq"], expect_seq(d, 4)), d
        assert c["probs"].dtype == torch.float64 and torch.equal(c["probs"], expect_probs(d, 4)), d
    # towards the episode's end the horizon shrinks (11 steps played of 12 at the last planned decision) and the shift follows it
    while e.steps_to_episode_end() > 4:
        e.step()
        ag.act(e)
    assert e.calls[-1]["K"] == 3 and ag.last_horizon == 3
    d = len(e.calls)
    assert torch.equal(e.calls[-1]["best_seq"], expect_seq(d - 1, 3)) and torch.equal(e.calls[-1]["probs"], expect_probs(d - 1, 3))
    e.step()
    ag.act(e)
    assert e.calls[-1]["K"] == 2 and torch.equal(e.calls[-1]["best_seq"], expect_seq(d, 2))
    e.step()
    ag.act(e)
    assert e.calls[-1]["K"] == 1 and torch.equal(e.calls[-1]["best_seq"], nothing.expand(1, 2, 3))
    assert torch.equal(e.calls[-1]["probs"], torch.full((1, 2, 3, 3), third, dtype=torch.float64))
    # one step left: no plan, do nothing
    e.step()
    n = len(e.calls)
    assert e.steps_to_episode_end() == 1
    assert torch.equal(ag.act(e), nothing.expand(2, 3)) and len(e.calls) == n and ag.last is None and ag.last_horizon == 0
    # the episode step goes backwards: both start afresh, and the decision counter goes on
    e.step()
    assert e.steps_to_episode_end() == 12
    ag.act(e)
    c = e.calls[-1]
    assert c["probs"] is None and c["best_seq"] is None and c["draw"] == n and c["K"] == 4
    e.step()
    ag.act(e)
    assert torch.equal(e.calls[-1]["best_seq"], expect_seq(n + 1, 4))
    e.t = 0      # ... also straight from a warm decision
    ag.act(e)
    assert e.calls[-1]["probs"] is None and e.calls[-1]["best_seq"] is None and e.calls[-1]["draw"] == n + 2
    # without warm start every decision starts afresh
    cold = CEMMPCAgent(6, 2, 3, 4, warm_start=False)
    e2 = _Stub()
    for _ in range(3):
        cold.act(e2)
        e2.step()
    assert all(c["probs"] is None and c["best_seq"] is None for c in e2.calls) and [c["draw"] for c in e2.calls] == [0, 1, 2]
