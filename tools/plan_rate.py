"""Measurement: SdcEngine.plan (one sdc_plan call: mark, per candidate rollout / score / rewind, select) beside SdcEngine.lookahead (the
same rollouts and rewinds driven from Python, the rewards summed with torch ops) for the same M = 4 candidates x K = 8 steps, in ONE
process, at 4 096 and at 32 768 envs (672-step episodes).  Device events around each call, one warm-up call, then the median, min and
max of nine calls; also plan with three info columns in the objective (the score kernel's LDS route).  One JSON line per size.  Run it
under `rocprofv3 --kernel-trace --stats -- python tools/plan_rate.py` for sdc_plan_score_kernel's and sdc_plan_select_kernel's own
time.

--cem: SdcEngine.plan_cem (one sdc_plan_cem call) at I = 3 iterations, M = 8 candidates, E = 2 elites, K = 8 steps beside the same
planner driven from Python -- per iteration torch sampling from the distributions, `plan`, topk, the refit as torch ops -- and beside
3 x the time of one `plan` of the same M and K; the same process, sizes and timing.  Under rocprofv3 as above for
sdc_cem_sample_kernel's and sdc_cem_refit_kernel's own time.

--groups: SdcEngine.plan_cem_groups (one sdc_plan_cem_groups call) at I = 3, K = 8, E = R / 8, G = 64 groups of R = 64 replicas (4 096
envs) and of R = 512 (32 768 envs), beside SdcEngine.plan_cem on a 64-env engine with M = 64 candidates -- as many samples per data
centre as the R = 64 case -- and beside three single-candidate `plan` calls at the groups' batch size (three 8-step rollouts, scores
and rewinds); the same process and timing.  Under rocprofv3 as above for sdc_cem_group_sample_kernel's and
sdc_cem_group_refit_kernel's own time.

--terms: one `plan` call at 4 096 envs, M = 8 candidates, K = 8 steps with no plan terms (sdc_plan_score_kernel), with 2 limits + 1
terminal column and with 8 + 8 (sdc_plan_score_terms_kernel: SdcEngine.set_plan_terms); the same process and timing, the three taken
in turn three times so that a drift of the machine shows as a spread of each.  On a revision without plan terms: the first alone."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from tools.clone_rate import EP
from tools.mark_rate import timed3

REPS = 9
M, K = 4, 8
CEM_I, CEM_M, CEM_E, CEM_K = 3, 8, 2, 8
COLUMNS = {"bat_CO2_footprint": -1e-3, "dc_water_usage": -1.0, "ls_tasks_dropped": -1.0}


def cem_in_python(eng, probs, best_seq, I, M, E):
    """the loop plan_cem replaces: per iteration sample from probs [K, N, 3, 3], score with `plan`, keep the best, refit to the elites"""
    K, N = probs.shape[0], probs.shape[1]
    ar = torch.arange(N, device=probs.device)
    for _ in range(I):
        draws = torch.multinomial(probs.reshape(-1, 3), M - 1, replacement=True)      # [K N 3, M-1]
        cand = torch.empty((M, K, N, 3), dtype=torch.int32, device=probs.device)
        cand[0] = best_seq
        cand[1:] = draws.reshape(K, N, 3, M - 1).permute(3, 0, 1, 2)
        score = eng.plan(cand).score
        elite = score.topk(E, dim=0).indices      # [E, N]
        best_seq = cand[elite[0], :, ar].permute(1, 0, 2).contiguous()
        picked = cand[elite, :, ar[None]].long()      # [E, N, K, 3]
        cnt = torch.zeros((N, K, 3, 3), dtype=torch.float64, device=probs.device)
        cnt.scatter_add_(3, picked.permute(1, 2, 3, 0), torch.ones((N, K, 3, E), dtype=torch.float64, device=probs.device))
        probs = (cnt / E).permute(1, 0, 2, 3).contiguous()
    return probs, best_seq


def main_cem():
    I, M, E, K = CEM_I, CEM_M, CEM_E, CEM_K
    for N in (4096, 32768):
        eng, _, _ = bench.build_engine(N, EP, 0, seed=99, debug_flags=0)
        eng.reset()
        g = torch.Generator(device="cpu").manual_seed(N)
        acts = torch.randint(0, 3, (8, N, 3), dtype=torch.int32, generator=g).cuda()
        for t in range(40):
            eng.step(acts[t % 8])
        cand = torch.randint(0, 3, (M, K, N, 3), dtype=torch.int32, generator=g).cuda()
        uniform = torch.full((K, N, 3, 3), 1.0 / 3.0, dtype=torch.float64, device=cand.device)
        nothing = torch.tensor([1, 1, 2], dtype=torch.int32, device=cand.device).expand(K, N, 3).contiguous()
        res = eng.plan_cem(K, I, M, E)      # (warm: the handle's buffers are allocated)
        eng.plan(cand)
        cem_in_python(eng, uniform, nothing, I, M, E)
        torch.cuda.synchronize()
        improved = int((res.best_score[-1] > res.best_score[0]).sum())
        cem = timed3(lambda: eng.plan_cem(K, I, M, E), REPS)
        loop = timed3(lambda: cem_in_python(eng, uniform, nothing, I, M, E), REPS)
        plan = timed3(lambda: eng.plan(cand), REPS)
        eng.step(acts[0])
        print(json.dumps(dict(what="plan_cem", n_envs=N, iterations=I, candidates=M, elites=E, steps=K, plan_cem_ms=cem[0],
                              plan_cem_ms_range=cem[1:], python_loop_ms=loop[0], python_loop_ms_range=loop[1:],
                              three_plans_ms=3 * plan[0], three_plans_ms_range=[3 * plan[1], 3 * plan[2]],
                              envs_improved_after_iteration_0=improved, step_kernel_after=eng.last_step_kernel())))
        eng.close()


def _warm_engine(N):
    eng, _, _ = bench.build_engine(N, EP, 0, seed=99, debug_flags=0)
    eng.reset()
    g = torch.Generator(device="cpu").manual_seed(N)
    acts = torch.randint(0, 3, (8, N, 3), dtype=torch.int32, generator=g).cuda()
    for t in range(40):
        eng.step(acts[t % 8])
    return eng, g


def main_groups():
    I, K, G = 3, 8, 64
    small, _ = _warm_engine(G)
    small.plan_cem(K, I, 64, 8)      # (warm: the handle's buffers are allocated)
    torch.cuda.synchronize()
    serial = timed3(lambda: small.plan_cem(K, I, 64, 8), REPS)
    print(json.dumps(dict(what="plan_cem", n_envs=G, iterations=I, candidates=64, elites=8, steps=K, plan_cem_ms=serial[0],
                          plan_cem_ms_range=serial[1:], step_kernel_after=small.last_step_kernel())))
    small.close()
    for R in (64, 512):
        N, E = G * R, R // 8
        eng, g = _warm_engine(N)
        eng.sync_groups(R)
        one = torch.randint(0, 3, (1, K, N, 3), dtype=torch.int32, generator=g).cuda()
        res = eng.plan_cem_groups(R, K, I, E)
        eng.plan(one)
        torch.cuda.synchronize()
        improved = int((res.best_score[-1] > res.best_score[0]).sum())
        grp = timed3(lambda: eng.plan_cem_groups(R, K, I, E), REPS)
        plan = timed3(lambda: eng.plan(one), REPS)
        eng.step(res.step_actions)
        print(json.dumps(dict(what="plan_cem_groups", n_envs=N, groups=G, group_size=R, iterations=I, elites=E, steps=K,
                              plan_cem_groups_ms=grp[0], plan_cem_groups_ms_range=grp[1:], three_single_candidate_plans_ms=3 * plan[0],
                              three_single_candidate_plans_ms_range=[3 * plan[1], 3 * plan[2]],
                              groups_improved_after_iteration_0=improved, step_kernel_after=eng.last_step_kernel())))
        eng.close()


TERMS_FEW = ({"dc_int_temperature": (None, 27.0, 10.0), "bat_SOC": (0.2, None, 5.0)}, {"ls_tasks_in_queue": -1e-3})
TERMS_FULL = ({"dc_int_temperature": (18.0, 27.0, 10.0), "bat_SOC": (0.2, 0.9, 5.0), "dc_crac_setpoint": (16.0, 22.0, 1.0),
               "dc_total_power_kW": (None, 1500.0, 1e-3), "ls_tasks_dropped": (None, 0.0, 2.0)},
              {"ls_tasks_in_queue": -1e-3, "ls_oldest_task_age": -0.1, "ls_overdue_penalty": -1.0, "bat_SOC": 1.0,
               "ls_norm_tasks_in_queue": -0.5, "ls_average_task_age": -0.1, "dc_int_temperature": -0.01, "bat_CO2_footprint": -1e-6})


def main_terms():
    N, M_, K_ = 4096, 8, 8
    eng, g = _warm_engine(N)
    cand = torch.randint(0, 3, (M_, K_, N, 3), dtype=torch.int32, generator=g).cuda()
    cases = [("no_terms", None)]
    if hasattr(eng, "set_plan_terms"):
        cases += [("limits_2_terminal_1", TERMS_FEW), ("limits_8_terminal_8", TERMS_FULL)]
    scores = {}
    for name, terms in cases:      # (warm: the handle's buffers, both score kernels' code)
        if terms is not None:
            eng.set_plan_terms(*terms)
        scores[name] = eng.plan(cand, info_weights=COLUMNS).score
    torch.cuda.synchronize()
    out = dict(what="plan_terms", n_envs=N, candidates=M_, steps=K_, objective_columns=len(COLUMNS))
    for turn in range(3):
        for name, terms in cases:
            if hasattr(eng, "set_plan_terms"):
                eng.set_plan_terms(*(terms or ()))
            out.setdefault(name + "_ms", []).append(timed3(lambda: eng.plan(cand, info_weights=COLUMNS), REPS))
    out["scores_differ_from_no_terms"] = {k: bool((v != scores["no_terms"]).any()) for k, v in scores.items() if k != "no_terms"}
    eng.step(cand[0, 0])
    out["step_kernel_after"] = eng.last_step_kernel()
    print(json.dumps(out))
    eng.close()


def main():
    if "--terms" in sys.argv[1:]:
        return main_terms()
    if "--cem" in sys.argv[1:]:
        return main_cem()
    if "--groups" in sys.argv[1:]:
        return main_groups()
    for N in (4096, 32768):
        eng, _, _ = bench.build_engine(N, EP, 0, seed=99, debug_flags=0)
        eng.reset()
        g = torch.Generator(device="cpu").manual_seed(N)
        acts = torch.randint(0, 3, (8, N, 3), dtype=torch.int32, generator=g).cuda()
        for t in range(40):
            eng.step(acts[t % 8])
        cand = torch.randint(0, 3, (M, K, N, 3), dtype=torch.int32, generator=g).cuda()
        ref, res = eng.lookahead(cand), eng.plan(cand)      # (warm: the handle's buffers are allocated; and the two routes agree)
        assert torch.equal(ref, res.returns)
        eng.plan(cand, info_weights=COLUMNS)
        torch.cuda.synchronize()
        look = timed3(lambda: eng.lookahead(cand), REPS)
        plan = timed3(lambda: eng.plan(cand), REPS)
        cols = timed3(lambda: eng.plan(cand, info_weights=COLUMNS), REPS)
        eng.step(acts[0])
        print(json.dumps(dict(what="plan", n_envs=N, candidates=M, steps=K, lookahead_ms=look[0], lookahead_ms_range=look[1:],
                              plan_ms=plan[0], plan_ms_range=plan[1:], plan_3_columns_ms=cols[0], plan_3_columns_ms_range=cols[1:],
                              step_kernel_after=eng.last_step_kernel())))
        eng.close()


if __name__ == "__main__":
    main()
