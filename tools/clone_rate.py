"""Measurement: sdc_clone_envs (SdcEngine.clone_envs) -- run it under `rocprofv3 --kernel-trace --stats -- python tools/clone_rate.py`
for sdc_clone_kernel's own time; this script prints the bytes each clone moves and host-side timings as JSON lines:
  * "clone": 16 384 pairs at 32 768 envs (state well beyond the 256 MiB Infinity Cache) and 64 sources -> 4 032 dst at 4 096 envs,
    672-step episodes: bytes read + written per call, the call's time between device events (median of REPS);
  * "state_dict_route": the host route a clone replaces at 4 096 envs -- state_dict(), copy the rows, load_state_dict() -- wall time;
  * "after_clone": five single steps right after a lock-step clone against five steps without one (device events, 32 768 envs)."""
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from dc_rl_amd import _lib as L

EP, REPS = 672, 9


def _define(name, fname):
    """a #define of the library's own sources (the batch sizes from which the mirrors exist): this count follows them"""
    m = re.search(r"#define %s (\d+)" % name, open(os.path.join(L.CSRC, fname)).read())
    assert m, (name, fname)
    return int(m.group(1))


def clone_bytes(eng, n_pairs):
    """bytes read + written by one clone of n_pairs pairs (sdc_clone.hpp ranges A, B, C), from the engine's own strides and the
    library's own thresholds (sdc_dispatch.hpp sdc_wide_mirrors: which arrays a batch has)"""
    N, E, cap = eng.n_envs, eng.episode_steps, eng.config["hist_cap"]
    per = (4 * L.HDR_DWORDS * 2 + 4 * eng.hist_stride + 4 * 4 * L.QWIN + 8 * eng.queue_stride + 2 * 8 * eng.lw +   # A: record, header,
           4 * L.N_AGENTS * L.OBS_PAD + 4 * L.SHARE_OBS_DIM)                                                        # ring ... obs rows
    if eng.config["n_dc_configs"] > 1:
        per += 8 * 32                                                                                                # A: config scalars
    if 8 * (E + 25 + eng.lw) <= 50 * 1024:
        per += (E + 1) * 4 * 32                                                                                      # B: feature rows
    if N % 64 == 0 and N >= _define("SDC_WIDE_MIN_ENVS", "sdc_dispatch.hpp"):                                          # C: the mirrors
        per += 4 * (eng.queue_stride + (cap if N >= _define("SDC_HIST_MIRROR_MIN_ENVS", "sdc_device.hpp") else 0))
    return 2 * per * n_pairs


def timed(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def engine(N):
    eng, _, _ = bench.build_engine(N, EP, 0, seed=99, debug_flags=0)
    eng.reset()
    g = torch.Generator(device="cpu").manual_seed(N)
    acts = torch.randint(0, 3, (8, N, 3), dtype=torch.int32, generator=g).cuda()
    for t in range(40):
        eng.step(acts[t % 8])
    torch.cuda.synchronize()
    return eng, acts


def main():
    out = []
    for N, src, dst in ((32768, np.arange(16384), np.arange(16384, 32768)),
                        (4096, np.arange(64), np.arange(64, 4096))):
        eng, acts = engine(N)
        s = np.resize(src, dst.shape)        # (64 sources cycled over the 4 032 dst)
        eng.clone_envs(s, dst)               # (warm: the staging buffers are allocated on the first call)
        ms = timed(lambda: eng.clone_envs(s, dst))
        nb = clone_bytes(eng, len(dst))
        out.append(dict(what="clone", n_envs=N, pairs=int(len(dst)), bytes=nb, event_ms=ms, event_TBps=nb / ms / 1e9,
                        kernel=eng.last_step_kernel()))
        if N == 32768:
            # five steps after a lock-step clone against five without (the same engine, alternated)
            def five():
                for t in range(5):
                    eng.step(acts[t])
            plain = timed(five, 5)
            after = []
            for _ in range(5):
                eng.clone_envs(s, dst)
                torch.cuda.synchronize()
                after.append(timed(five, 1))
            out.append(dict(what="after_clone", n_envs=N, five_steps_ms=plain, five_steps_after_clone_ms=float(np.median(after)),
                            kernel=eng.last_step_kernel()))
        else:
            t0 = time.perf_counter()
            sd = eng.state_dict()
            for k, v in sd.items():
                if k != "meta":
                    v[dst] = v[s]
            eng.load_state_dict(sd)
            torch.cuda.synchronize()
            out.append(dict(what="state_dict_route", n_envs=N, pairs=int(len(dst)), wall_ms=(time.perf_counter() - t0) * 1e3))
        eng.close()
    for r in out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
