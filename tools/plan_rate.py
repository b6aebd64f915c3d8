"""Measurement: SdcEngine.plan (one sdc_plan call: mark, per candidate rollout / score / rewind, select) beside SdcEngine.lookahead (the
same rollouts and rewinds driven from Python, the rewards summed with torch ops) for the same M = 4 candidates x K = 8 steps, in ONE
process, at 4 096 and at 32 768 envs (672-step episodes).  Device events around each call, one warm-up call, then the median, min and
max of nine calls; also plan with three info columns in the objective (the score kernel's LDS route).  One JSON line per size.  Run it
under `rocprofv3 --kernel-trace --stats -- python tools/plan_rate.py` for sdc_plan_score_kernel's and sdc_plan_select_kernel's own
time."""
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
COLUMNS = {"bat_CO2_footprint": -1e-3, "dc_water_usage": -1.0, "ls_tasks_dropped": -1.0}


def main():
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
