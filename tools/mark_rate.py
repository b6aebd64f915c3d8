"""Measurement: mark / rewind (SdcEngine.mark / rewind over sdc_mark_envs / sdc_rewind_envs) against the snapshot route -- run it under
`rocprofv3 --kernel-trace --stats -- python tools/mark_rate.py` for sdc_mark_save_kernel's and sdc_mark_rewind_kernel's own time; this
script prints, as JSON lines, for every env of a batch at 4 096 and 32 768 envs (672-step episodes), in ONE process:
  * "mark" / "rewind" for max_steps 16 and 64, "save" / "restore" of the same batch: the bytes one call reads + writes, its time between
    device events (median, min and max of REPS calls after a warm-up call), the rate;
  * "after_rewind" (32 768 envs): five single steps right after a whole-batch rewind against the same five steps without one;
  * "lookahead" (4 096 envs): M = 4 candidates x K = 8 steps through SdcEngine.lookahead against the same loop written with
    snapshot / restore, wall time with a device synchronisation at the end (median of REPS)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from tools.clone_rate import EP, REPS, _define
from tools.snapshot_rate import call_bytes


def timed3(fn, reps=REPS):
    """(median, min, max) ms between device events around fn()"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def mark_bytes(eng, K, rewind):
    """bytes read + written by one call over every env: the row's used part both ways (sdc_mark.hpp range A), and for a rewind the
    mirrors' dwords (range M: the row's record fields, cum values and keys read again, the mirror dwords written) and the closed
    loop's copy of obs (none here: no actor is set)"""
    N = eng.n_envs
    per = 2 * (1964 + 12 * K)
    if rewind and N % 64 == 0 and N >= _define("SDC_WIDE_MIN_ENVS", "sdc_dispatch.hpp"):
        mirrors = 2 if N >= _define("SDC_HIST_MIRROR_MIN_ENVS", "sdc_device.hpp") else 1
        per += 12 + 8 * K * mirrors
    return per * N


def wall(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


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
        for K in (16, 64):
            mk = eng.mark(max_steps=K)      # (warm)
            eng.rewind(mk)
            ms = timed3(lambda: eng.mark(max_steps=K))
            nb = mark_bytes(eng, K, False)
            out.append(dict(what="mark", n_envs=N, max_steps=K, row_bytes=int(mk.rows.shape[1]), bytes=nb, event_ms=ms[0],
                            event_ms_range=ms[1:], event_TBps=nb / ms[0] / 1e9))
            mk = eng.mark(max_steps=K)
            ms = timed3(lambda: eng.rewind(mk))
            nb = mark_bytes(eng, K, True)
            out.append(dict(what="rewind", n_envs=N, max_steps=K, bytes=nb, event_ms=ms[0], event_ms_range=ms[1:],
                            event_TBps=nb / ms[0] / 1e9))
        snap = eng.snapshot()               # (warm: the staging buffers are allocated on the first call)
        eng.restore(snap)
        ms = timed3(lambda: eng.snapshot())
        nb = call_bytes(eng, False)
        out.append(dict(what="save", n_envs=N, row_bytes=int(snap.rows.shape[1]), bytes=nb, event_ms=ms[0], event_ms_range=ms[1:],
                        event_TBps=nb / ms[0] / 1e9))
        ms = timed3(lambda: eng.restore(snap))
        nb = call_bytes(eng, True)
        out.append(dict(what="restore", n_envs=N, bytes=nb, event_ms=ms[0], event_ms_range=ms[1:], event_TBps=nb / ms[0] / 1e9))
        del snap

        def five():
            for t in range(5):
                eng.step(acts[t])
        if N == 32768:
            mk = eng.mark(max_steps=16)
            plain, after = [], []
            for _ in range(5):          # (the same five steps from the same state, with and without a rewind in front, alternated)
                eng.rewind(mk)
                torch.cuda.synchronize()
                plain.append(timed3(five, 1)[0])
                kernel = eng.last_step_kernel()
                eng.rewind(mk)
                torch.cuda.synchronize()
                after.append(timed3(lambda: (eng.rewind(mk), five()), 1)[0])
            out.append(dict(what="after_rewind", n_envs=N, five_steps_ms=float(np.median(plain)),
                            rewind_and_five_steps_ms=float(np.median(after)), kernel=kernel))
        else:
            M, K = 4, 8
            cand = torch.randint(0, 3, (M, K, N, 3), dtype=torch.int32, generator=g).cuda()

            def by_snapshot():
                snap = eng.snapshot()
                ret = torch.empty((M, N, 3), dtype=torch.float64, device=eng.device)
                for c in range(M):
                    rew = eng.rollout(cand[c])[2]
                    ret[c].copy_(rew[0])
                    for k in range(1, K):
                        ret[c].add_(rew[k])
                    eng.restore(snap)
                return ret
            r1, r2 = eng.lookahead(cand), by_snapshot()      # (warm; and the two routes agree)
            assert torch.equal(r1, r2)
            a, b = wall(lambda: eng.lookahead(cand)), wall(by_snapshot)
            out.append(dict(what="lookahead", n_envs=N, candidates=M, steps=K, mark_rewind_ms=a[0], mark_rewind_ms_range=a[1:],
                            snapshot_restore_ms=b[0], snapshot_restore_ms_range=b[1:]))
        eng.close()
    for r in out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
