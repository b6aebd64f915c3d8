"""Measurement: one 672-step episode of 64 and of 4 096 envs under receding-horizon control with the cross-entropy method (H = 8, M = 8,
E = 2, I = 3), two ways --
  call   SdcEngine.rollout_cem_stats (one sdc_rollout_cem_stats call: per decision sdc_mpc_start_kernel, sdc_plan_cem's launches,
         sdc_mpc_fold_kernel, a one-step rollout and sdc_stats_reduce_kernel, with no Python in between);
  loop   the route it replaces: a Python loop of `CEMMPCAgent.act` (the horizon cut, the torch ops of the warm start, `plan_cem`) and a
         one-step `rollout_stats(..., into=)`.  It uses nothing this call added, so it runs from a checkout without it as well.
Device events around each episode, one warm-up episode per route, then the median, min and max of nine.  `--route both` (the default)
alternates the two routes episode by episode in one process; `--route call` / `--route loop` time one of them, for a session that
alternates two checkouts.  Every episode starts at an episode's first step (the auto-reset of the one before).  One JSON line per size.
`--groups R [R ...]`: the replica-group planner instead -- G = 64 groups of R replicas (64 R envs), E = R / 8, the same H and I --, the
call SdcEngine.rollout_cem_groups_stats (one sdc_rollout_cem_groups_stats call per episode, the sync inside it), the loop
`GroupCEMMPCAgent.act` (which syncs the groups at an episode's first step) and a one-step `rollout_stats(..., into=)`.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/mpc_eval_rate.py --route call` for the kernels' own times."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from dc_rl_amd.agents import CEMMPCAgent, GroupCEMMPCAgent
from tools.clone_rate import EP

REPS = 9
CEM = dict(n_candidates=8, n_elite=2, n_iters=3, horizon=8, seed=99)
GROUPS = 64      # --groups: data centres planned for


def python_loop(eng, agent):
    st = None
    for _ in range(EP):
        st = eng.rollout_stats(agent.act(eng)[None], into=st)
    return st


def one_call(eng, agent):
    return agent.rollout_stats(eng, EP)


def episode_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("both", "call", "loop"), default="both")
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--reps", type=int, default=REPS, help="timed episodes per route (a profiler run wants few)")
    ap.add_argument("--groups", type=int, nargs="+", default=None, metavar="R",
                    help=f"the replica-group planner: {GROUPS} groups of R replicas each, E = R / 8 (--envs is ignored)")
    args = ap.parse_args()
    routes = [r for r in ("call", "loop") if args.route in ("both", r)]
    fns = dict(call=one_call, loop=python_loop)
    for size in (args.groups or args.envs):
        R = size if args.groups else None
        N = GROUPS * R if R else size
        eng, _, _ = bench.build_engine(N, EP, 0, seed=99, debug_flags=0)
        eng.reset()
        if R:
            cem = dict(n_elite=R // 8, n_iters=CEM["n_iters"], horizon=CEM["horizon"], seed=CEM["seed"])
            agents = {r: GroupCEMMPCAgent(R, **cem) for r in routes}
        else:
            cem = CEM
            agents = {r: CEMMPCAgent(**CEM) for r in routes}
        for r in routes:      # (warm: the handle's buffers are allocated; every route runs one episode)
            st = fns[r](eng, agents[r])
        torch.cuda.synchronize()
        assert eng.steps_to_episode_end() == EP and int(st.steps.min()) == EP
        ts = {r: [] for r in routes}
        for _ in range(args.reps):      # alternated: an episode of each route in turn
            for r in routes:
                ts[r].append(episode_ms(lambda: fns[r](eng, agents[r])))
        out = dict(what="rollout_cem_groups_stats" if R else "rollout_cem_stats", n_envs=N, episode_steps=EP, reps=args.reps,
                   **({"groups": GROUPS, "group_size": R} if R else {}), **{k: v for k, v in cem.items() if k != "seed"})
        for r in routes:
            out[f"{r}_ms"] = float(np.median(ts[r]))
            out[f"{r}_ms_range"] = [float(min(ts[r])), float(max(ts[r]))]
        if len(routes) == 2:
            out["call_over_loop_min"] = out["call_ms"] / out["loop_ms_range"][0]
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
