"""Measurement: env snapshots (SdcEngine.snapshot / restore over sdc_snapshot_envs / sdc_restore_envs) -- run it under
`rocprofv3 --kernel-trace --stats -- python tools/snapshot_rate.py` for sdc_snapshot_save_kernel's and sdc_snapshot_restore_kernel's own
time; this script prints, as JSON lines, for every env of a batch at 4 096 and 32 768 envs (672-step episodes):
  * "save" / "restore": the bytes one call reads + writes, its time between device events (median of REPS), the rate;
  * "after_restore": five single steps right after a whole-batch rewind against the same five steps without one (device events);
  * "state_dict_route" (4 096 envs): the host route a rewind replaces -- state_dict(), load_state_dict() -- wall time."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from tools.clone_rate import EP, REPS, _define, timed


def call_bytes(eng, restore):
    """bytes read + written by one call over every env: the row both ways (sdc_snapshot.hpp ranges A, B), and for a restore the
    mirrors (range C: the cum column of the queue table and the ring read again, the mirror rows written) and the closed loop's copy"""
    N, cap = eng.n_envs, eng.config["hist_cap"]
    per = 2 * int(eng.lib.sdc_snapshot_row_bytes(eng._h))
    if restore and N % 64 == 0 and N >= _define("SDC_WIDE_MIN_ENVS", "sdc_dispatch.hpp"):
        rows = eng.queue_stride + (cap if N >= _define("SDC_HIST_MIRROR_MIN_ENVS", "sdc_device.hpp") else 0)
        per += 8 * eng.queue_stride + 4 * rows      # (range C reads whole 16-byte pieces of the queue table: both columns)
    return per * N


def main():
    out = []
    for N in (4096, 32768):
        eng, _, _ = bench.build_engine(N, EP, 0, seed=99, debug_flags=0)
        eng.reset()
        g = torch.Generator(device="cpu").manual_seed(N)
        acts = torch.randint(0, 3, (8, N, 3), dtype=torch.int32, generator=g).cuda()
        for t in range(40):
            eng.step(acts[t % 8])
        torch.cuda.synchronize()
        snap = eng.snapshot()           # (warm: the staging buffers are allocated on the first call)
        eng.restore(snap)
        ms = timed(lambda: eng.snapshot())
        nb = call_bytes(eng, False)
        out.append(dict(what="save", n_envs=N, row_bytes=int(snap.rows.shape[1]), bytes=nb, event_ms=ms, event_TBps=nb / ms / 1e9))
        ms = timed(lambda: eng.restore(snap))
        nb = call_bytes(eng, True)
        out.append(dict(what="restore", n_envs=N, bytes=nb, event_ms=ms, event_TBps=nb / ms / 1e9, kernel=eng.last_step_kernel()))

        def five():
            for t in range(5):
                eng.step(acts[t])
        snap = eng.snapshot()
        plain, after = [], []
        for _ in range(5):          # (the same five steps from the same state, with and without a rewind in front, alternated)
            eng.restore(snap)
            torch.cuda.synchronize()
            plain.append(timed(five, 1))
            kernel = eng.last_step_kernel()
            eng.restore(snap)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.restore(snap)
            five()
            b.record()
            torch.cuda.synchronize()
            after.append(a.elapsed_time(b))
        out.append(dict(what="after_restore", n_envs=N, five_steps_ms=float(np.median(plain)),
                        restore_and_five_steps_ms=float(np.median(after)), kernel=kernel))
        if N == 4096:
            t0 = time.perf_counter()
            eng.load_state_dict(eng.state_dict())
            torch.cuda.synchronize()
            out.append(dict(what="state_dict_route", n_envs=N, wall_ms=(time.perf_counter() - t0) * 1e3))
        del snap
        eng.close()
    for r in out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
