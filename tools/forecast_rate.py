"""Measurement: SdcEngine.plan (one sdc_plan call) of M = 4 candidates x K = 8 steps without a plan forecast and with a persistence
forecast on all four channels (SdcEngine.set_plan_forecast: one sdc_forecast_fill_kernel launch and two sdc_forecast_swap_kernel
launches more per call), in ONE process, at 4 096 and at 32 768 envs (672-step episodes).  Device events around each call, one warm-up
call of each, then the median, min and max of nine calls; the two taken in turn twice, so that a drift of the machine shows as a spread
of each.  One JSON line per size.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/forecast_rate.py` for the two
kernels' own time."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.mark_rate import timed3
from tools.plan_rate import K, M, REPS, _warm_engine

PERSISTENCE = dict(workload="persistence", carbon="persistence", temperature="persistence", wet_bulb="persistence")


def main():
    for N in (4096, 32768):
        eng, g = _warm_engine(N)
        cand = torch.randint(0, 3, (M, K, N, 3), dtype=torch.int32, generator=g).cuda()
        oracle = eng.plan(cand)      # (warm: the handle's buffers are allocated, the kernels' code is loaded)
        eng.set_plan_forecast(**PERSISTENCE)
        under = eng.plan(cand)
        torch.cuda.synchronize()
        out = dict(what="plan_forecast", n_envs=N, candidates=M, steps=K)
        for turn in range(2):
            for name, forecast in (("no_forecast", {}), ("persistence", PERSISTENCE)):
                eng.set_plan_forecast(**forecast)
                out.setdefault(name + "_ms", []).append(timed3(lambda: eng.plan(cand), REPS))
        out["overhead_ms"] = [round(p[0] - n[0], 4) for n, p in zip(out["no_forecast_ms"], out["persistence_ms"])]
        out["scores_differ"] = bool((under.score != oracle.score).any())
        out["choices_differ"] = int((under.best != oracle.best).sum())
        eng.set_plan_forecast(None)
        eng.step(cand[0, 0])
        out["step_kernel_after"] = eng.last_step_kernel()
        print(json.dumps(out))
        eng.close()


if __name__ == "__main__":
    main()
