"""What the planner tests share (sdc_plan, sdc_plan_cem, sdc_plan_cem_groups, sdc_rollout_stats): on the CPU side the entry point's
declaration, the ctypes mirrors' layout and the kernels' resource usage; on the GPU side the twin engines, the refusal rig and the CEM
arithmetic restated; and the engine stub the agents' host logic runs against.  A plain module: the test files import from here, not from
one another."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from dc_rl_amd import _lib as L

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "sustaindc_hip.h")
EP = 96
RSV = L.INFO_IDX["reserved"]
OBJ = dict(reward_weights=(0.5, 2.0, -1.0), gamma=0.9, info_weights={"bat_CO2_footprint": -1e-3, "dc_water_usage": -0.5})


# ---- CPU side ---------------------------------------------------------------------------------------------------------------------
def entry_point_header(fn, args, source):
    """`fn` is declared with the argument names `args`, exported and bound with the ABI still at 313, and `source` is one of the
    library's sources; -> the header without its comments, for the caller's own #defines"""
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define SDC_ABI_VERSION 313\b", hdr)
    decl = re.search(r"\bint %s\(([^)]*)\);" % fn, hdr)
    assert decl and [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == args, decl
    assert fn in L.EXPORTS
    assert L.ABI_VERSION == 313 and source in L.SOURCES
    L.build()
    lib = C.CDLL(L.LIB_PATH)
    assert lib.sdc_version() == 313
    assert hasattr(lib, fn)
    assert len(getattr(L.load(), fn).argtypes) == len(args)
    return hdr


def assert_c_layout(tmp_path, c_struct, mirror, members):
    """the ctypes class `mirror` has the size, the member offsets and the member order the C compiler gives `c_struct`"""
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
           f'  printf("sizeof %zu\\n", sizeof({c_struct}));']
    src += [f'  printf("{m} %zu\\n", offsetof({c_struct}, {m}));' for m in members]
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-o", exe, str(c)], check=True)
    out = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(mirror)
    for m in members:
        assert int(out[m]) == getattr(mirror, m).offset, m
    assert [f[0] for f in mirror._fields_] == members


def kernel_resources(source):
    """`source` cross-compiled for gfx950 with the library's flags -> {kernel: {remark: value}} of the compiler's resource-usage remarks"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = [f for f in L.HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc] + flags + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", source,
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
    return per


def assert_no_scratch_or_spills(per, kernels):
    assert set(per) == set(kernels), sorted(per)
    for k, u in per.items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)


class AgentStub:
    """What the CEM agents' `act` and `rollout_stats` ask of an engine, on the CPU: sync_groups, plan_cem and plan_cem_groups record
    their arguments; the plans answer with tensors that tell the step and the decision apart (best_seq[k] = 100 d + 10 k + agent,
    probs[k] = d + k / 16 + (agent, action) / 256, step_actions = best_seq[0] of the env's group); rollout_cem_stats and
    rollout_cem_groups_stats: below."""

    def __init__(self, n_envs=2, episode_steps=12):
        import torch
        self.n_envs, self.device = n_envs, torch.device("cpu")
        self.config = dict(auto_reset=True, episode_steps=episode_steps)
        self.t, self.calls, self.syncs, self.loops = 0, [], [], []

    def steps_to_episode_end(self):
        return self.config["episode_steps"] - self.t

    def step(self):
        self.t = (self.t + 1) % self.config["episode_steps"]

    def _answer(self, K, lead, n_iters, probs, best_seq, **rec):
        import torch
        self.calls.append(dict(K=K, probs=None if probs is None else probs.clone(), best_seq=None if best_seq is None else best_seq.clone(),
                               n_iters=n_iters, **rec))
        d = len(self.calls)
        k = torch.arange(K).view(K, 1, 1)
        seq = (100 * d + 10 * k + torch.arange(3).view(1, 1, 3)).expand(K, lead, 3).to(torch.int32).contiguous()
        p = (d + k.view(K, 1, 1, 1) / 16.0 + torch.arange(9).view(1, 1, 3, 3) / 256.0).expand(K, lead, 3, 3).to(torch.float64).contiguous()
        return seq, torch.zeros((n_iters, lead), dtype=torch.float64), p

    def plan_cem(self, K, n_iters, M, E, *, probs, best_seq, draw, **kw):
        from dc_rl_amd.engine import CEMResult
        seq, score, p = self._answer(K, self.n_envs, n_iters, probs, best_seq, draw=draw, M=M, E=E, **kw)
        return CEMResult(seq[0].clone(), seq, score, p, None, None)

    def sync_groups(self, R):
        self.syncs.append((len(self.calls), R))

    def plan_cem_groups(self, R, K, n_iters, E, *, probs, best_seq, draw, **kw):
        from dc_rl_amd.engine import GroupCEMResult
        seq, score, p = self._answer(K, self.n_envs // R, n_iters, probs, best_seq, R=R, draw=draw, E=E, **kw)
        return GroupCEMResult(seq[0].clone(), seq[0].repeat_interleave(R, dim=0), seq, score, p, None, None)

    # The closed-loop calls of the agents' `rollout_stats`: recorded in `loops` with every keyword they were given (probs and best_seq as
    # copies); `refuse`: raise as the engine refuses, nothing moved; else the batch moves n_steps, the caller's probs / best_seq are
    # filled with the call's number and go back in an MPCCarry of `carry` = (steps, planned)
    refuse, carry = False, (0, 0)

    def _loop(self, n_steps, H, probs, best_seq, **rec):
        from dc_rl_amd.engine import MPCCarry
        self.loops.append(dict(n_steps=n_steps, H=H, probs=probs.clone(), best_seq=best_seq.clone(), **rec))
        if self.refuse:
            raise ValueError("refused")
        self.t = (self.t + n_steps) % self.config["episode_steps"]
        res = type("Res", (), {})()
        res.mpc = MPCCarry(probs.fill_(len(self.loops)), best_seq.fill_(len(self.loops)), *self.carry, None, None)
        return res

    def rollout_cem_stats(self, n_steps, H, n_iters, M, E, *, probs, best_seq, **kw):
        return self._loop(n_steps, H, probs, best_seq, n_iters=n_iters, M=M, E=E, **kw)

    def rollout_cem_groups_stats(self, n_steps, R, H, n_iters, E, *, probs, best_seq, **kw):
        return self._loop(n_steps, H, probs, best_seq, n_iters=n_iters, R=R, E=E, **kw)


# ---- GPU side ---------------------------------------------------------------------------------------------------------------------
def _twins(N, n=2, history=20, seed=21, policy=None, **kw):
    """n engines with one seed after the same `history` random steps (built-in policies: steps without actions); -> (engines, the
    generator for what follows)"""
    import torch
    from tests.test_gpu_clone import _acts
    from tests.test_gpu_mark import _mk
    if policy is not None:
        kw["policy"] = policy
    engs = [_mk(N, ep=EP, seed=seed, **kw) for _ in range(n)]
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(history):
        x = None if policy is not None else _acts(N, g)
        for e in engs:
            e.step(x)
    return engs, g


def _outputs(e):
    return {nm: getattr(e, nm).clone() for nm in ("obs", "share_obs", "rew", "done", "info", "final_obs")}


def refused(eng, match, call):
    """call() raises a ValueError that says `match` and leaves the engine as it was: every state array and output buffer to the bit, the
    steps left in the episode"""
    import torch
    from tests.test_gpu_mark import _grab
    before, outs, left = _grab(eng), _outputs(eng), eng.steps_to_episode_end()
    with pytest.raises(ValueError, match=match):
        call()
    after = _grab(eng)
    for k, x in before.items():
        assert np.array_equal(x, after[k]), (match, k)
    for nm, x in outs.items():
        assert torch.equal(getattr(eng, nm).view(torch.uint8), x.view(torch.uint8)), (match, nm)
    assert eng.steps_to_episode_end() == left


def objective(n_cols, col0):
    o = L.SdcPlanObjective()
    o.reward_weight[:] = [1.0, 1.0, 1.0]
    o.gamma, o.n_cols = 1.0, n_cols
    o.col[0] = col0
    return o


def refusal_engines(N, alongside=0):
    """The engines the refusal tests run on, episodes of 48 steps: `a` 10 steps in (38 left), then `alongside` more that took the same
    10 steps, `fresh` never reset, `verify` in verify mode, `late` without auto-reset 46 steps in (2 left)"""
    import torch
    from tests.test_gpu_clone import _acts
    from tests.test_gpu_mark import _mk
    stepped = [_mk(N, ep=48) for _ in range(1 + alongside)]
    fresh = _mk(N, ep=48, reset=False)
    verify = _mk(N, ep=48, debug_flags=L.DEBUG_VERIFY)
    late = _mk(N, ep=48, auto_reset=False)
    g = torch.Generator(device="cpu").manual_seed(5)
    for _ in range(10):
        x = _acts(N, g)
        for e in stepped:
            e.step(x)
    for _ in range(46):
        late.step(_acts(N, g))
    return stepped + [fresh, verify, late]


def planner_refusals(plan, too_long, a, fresh, verify, late):
    """What every planner refuses as sdc_plan does, plan(engine, K, **objective arguments) the planner's call with horizon K: the
    horizon (`too_long`: the wording), auto-reset, past the end, no reset, verify mode, gamma, info keys, reward weights"""
    refused(a, too_long, lambda: plan(a, L.MARK_MAX_STEPS + 1))
    refused(a, "auto-reset", lambda: plan(a, 38))      # (38 steps left: the last one would reset)
    refused(late, "past the end", lambda: plan(late, 3))
    refused(fresh, "sdc_reset must be called first", lambda: plan(fresh, 2))
    refused(verify, "verify mode", lambda: plan(verify, 2))
    for bad in (0.0, -0.5, 1.5, float("nan")):
        refused(a, "gamma", lambda: plan(a, 3, gamma=bad))
    refused(a, "not an info column", lambda: plan(a, 3, info_weights={"no_such_key": 1.0}))
    refused(a, "at most 8", lambda: plan(a, 3, info_weights={k: 1.0 for k in L.INFO_COLS[:9]}))
    refused(a, "three numbers", lambda: plan(a, 3, reward_weights=(1.0, 1.0)))


def sample_ref(probs, M_, seed, draw, it, base=0, fixed=(-1, -1, -1)):
    """candidates 1 .. M-1 [M-1, K, N, 3] by the header's rule: one philox4x32_10 block per (m, k, n), counter (m K + k, base + n, draw,
    (it << 16) | 0xCE3D), key (seed lo, seed hi); u = word * 2^-32; action = (u >= p0) + (u >= p0 + p1).  For sdc_plan_cem_groups read
    "candidate m of env n" as "replica r of group g"."""
    from tests import reset_ref as RR
    p = probs.cpu().numpy()
    K_, N_ = p.shape[0], p.shape[1]
    m = np.arange(1, M_, dtype=np.uint64)[:, None, None]
    k = np.arange(K_, dtype=np.uint64)[None, :, None]
    n = np.arange(N_, dtype=np.uint64)[None, None, :]
    words = RR.philox4x32_10(m * np.uint64(K_) + k, np.uint64(base) + n, draw, (it << 16) | 0xCE3D, seed & 0xFFFFFFFF, seed >> 32)
    out = np.empty((M_ - 1, K_, N_, 3), dtype=np.int32)
    for a in range(3):
        u = np.asarray(words[a]).astype(np.float64) * 2.0 ** -32
        p0 = p[None, :, :, a, 0]
        p01 = p0 + p[None, :, :, a, 1]
        out[..., a] = (u >= p0).astype(np.int32) + (u >= p01).astype(np.int32)
        if fixed[a] >= 0:
            out[..., a] = fixed[a]
    return out


def refit_ref(cand, score, probs, best_seq, E_, alpha, p_min, fixed=(-1, -1, -1)):
    """the header's REFIT from one iteration's candidates [M, K, N, 3] and scores [M, N] (replicas [R, K, G, 3], [R, G]), in torch fp64,
    one operation per tensor op (no fused multiply-adds): -> (elite [M, N], best [N], best_seq, best_score [N], probs).  t_j = cnt_j / E
    divides by a TENSOR that holds E: torch divides a CUDA tensor by a Python scalar as a multiplication by the scalar's reciprocal,
    which is an ulp off the IEEE quotient for e.g. 5 / 21; tensor / tensor is the IEEE division the header states."""
    import torch
    M_, K_, N_, _ = cand.shape
    dev = cand.device
    c = torch.arange(M_, device=dev)
    # [c, c', n]: c' outranks c
    over = (score[None, :, :] > score[:, None, :]) | ((score[None, :, :] == score[:, None, :]) & (c[None, :, None] < c[:, None, None]))
    rank = over.sum(1)
    elite = rank < E_
    assert bool(((rank == 0).sum(0) == 1).all())
    best = (rank == 0).int().argmax(0)
    ar = torch.arange(N_, device=dev)
    winner = cand[best, :, ar].permute(1, 0, 2)      # [K, N, 3]
    new_seq = torch.where((best != 0)[None, :, None], winner, best_seq)
    best_score = score[best, ar]
    hit = (cand[..., None] == torch.arange(3, device=dev, dtype=cand.dtype)) & elite[:, None, :, None, None]      # [M, K, N, 3, 3]
    cnt = hit.sum(0).double()
    t = cnt / torch.full_like(cnt, float(E_))
    take = 1.0 - alpha
    q = probs * alpha + t * take
    q = torch.maximum(q, torch.tensor(p_min, dtype=torch.float64, device=dev))
    s = (q[..., 0] + q[..., 1]) + q[..., 2]
    p = q / s[..., None]
    for a in range(3):
        if fixed[a] >= 0:
            p[:, :, a] = probs[:, :, a]
    return elite, best, new_seq, best_score, p
