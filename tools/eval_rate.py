"""Measurement: one 672-step episode of 4 096 and of 32 768 envs, three ways in ONE process --
  rollout_stats   SdcEngine.rollout_stats (one sdc_rollout_stats call: rollouts into the handle's output block in chunks, one launch of
                  sdc_stats_reduce_kernel per chunk);
  python_loop     the route it replaces: a Python loop of `rollout` chunks of the same length, each chunk's info and rew reduced with
                  torch.sum / amin / amax and a count of positive values into fp64 accumulators;
  bare_rollouts   sdc_rollout calls of the same chunks into a preallocated block, nothing reduced: the floor.
Device events around each episode, one warm-up episode each, then the median, min and max of nine.  Every episode starts at an episode's
first step (the auto-reset of the one before).  One JSON line per size, with the chunk length and the bytes the reduce kernel reads per
episode (188 B per env-step).  Run it under `rocprofv3 --kernel-trace --stats -- python tools/eval_rate.py` for
sdc_stats_reduce_kernel's own time."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from dc_rl_amd import _lib as L
from tools.clone_rate import EP
from tools.mark_rate import timed3

REPS = 9
CAP = 256 << 20      # csrc/sdc_plan.hpp SDC_PLAN_SCRATCH_BYTES


def block_bytes(N, steps):
    """csrc/sdc_plan.hpp sdc_plan_block: the output block's size for `steps` steps of N envs"""
    up = lambda x: (x + 255) // 256 * 256
    o = up(steps * N * 4 * L.N_AGENTS * L.OBS_PAD)
    o = up(o + steps * N * 4 * L.SHARE_OBS_DIM)
    o = up(o + steps * N * 4 * L.N_AGENTS)
    o = up(o + steps * N * 4 * L.INFO_DIM)
    o = up(o + steps * N)
    return up(o + N * 4 * L.N_AGENTS * L.OBS_PAD)


def chunk_steps(N, K):
    """csrc/sdc_plan.hpp sdc_plan_steps_fit"""
    s = K
    while s > 1 and block_bytes(N, s) > CAP:
        s -= 1
    return s


def python_loop(eng, acts, chunk):
    N, dev = eng.n_envs, eng.device
    s = torch.zeros((N, L.INFO_DIM), dtype=torch.float64, device=dev)
    npos = torch.zeros((N, L.INFO_DIM), dtype=torch.float64, device=dev)
    lo = torch.full((N, L.INFO_DIM), float("inf"), dtype=torch.float32, device=dev)
    hi = torch.full((N, L.INFO_DIM), float("-inf"), dtype=torch.float32, device=dev)
    ret = torch.zeros((N, 3), dtype=torch.float64, device=dev)
    for k0 in range(0, acts.shape[0], chunk):
        o = eng.rollout(acts[k0:k0 + chunk])
        rew, info = o[2], o[4]
        s += info.sum(0, dtype=torch.float64)
        lo = torch.minimum(lo, info.amin(0))
        hi = torch.maximum(hi, info.amax(0))
        npos += (info > 0).sum(0)
        ret += rew.sum(0, dtype=torch.float64)
    return s, lo, hi, npos, ret


def bare_rollouts(eng, acts, chunk, block):
    p = lambda x: C.c_void_p(x.data_ptr())
    for k0 in range(0, acts.shape[0], chunk):
        a = acts[k0:k0 + chunk]
        L.check(eng.lib.sdc_rollout(eng._h, int(a.shape[0]), p(a), p(block["obs"]), p(block["share"]), p(block["rew"]), p(block["done"]),
                                    p(block["info"]), p(eng.final_obs), None, eng._stream()))


def main():
    for N in (4096, 32768):
        eng, _, _ = bench.build_engine(N, EP, 0, seed=99, debug_flags=0)
        eng.reset()
        g = torch.Generator(device="cpu").manual_seed(N)
        acts = torch.randint(0, 3, (EP, N, 3), dtype=torch.int32, generator=g).cuda()
        chunk = chunk_steps(N, EP)
        kw = dict(dtype=torch.float32, device=eng.device)
        block = dict(obs=torch.empty((chunk, N, L.N_AGENTS, L.OBS_PAD), **kw), share=torch.empty((chunk, N, L.SHARE_OBS_DIM), **kw),
                     rew=torch.empty((chunk, N, L.N_AGENTS), **kw), info=torch.empty((chunk, N, L.INFO_DIM), **kw),
                     done=torch.empty((chunk, N), dtype=torch.uint8, device=eng.device))
        st = eng.rollout_stats(acts)      # (warm: the handle's block is allocated; every route runs one episode)
        python_loop(eng, acts, chunk)
        bare_rollouts(eng, acts, chunk, block)
        torch.cuda.synchronize()
        assert eng.steps_to_episode_end() == EP and int(st.steps.min()) == EP
        stats = timed3(lambda: eng.rollout_stats(acts), REPS)
        loop = timed3(lambda: python_loop(eng, acts, chunk), REPS)
        bare = timed3(lambda: bare_rollouts(eng, acts, chunk, block), REPS)
        print(json.dumps(dict(what="rollout_stats", n_envs=N, episode_steps=EP, chunk_steps=chunk, chunks=-(-EP // chunk),
                              rollout_stats_ms=stats[0], rollout_stats_ms_range=stats[1:], python_loop_ms=loop[0],
                              python_loop_ms_range=loop[1:], bare_rollouts_ms=bare[0], bare_rollouts_ms_range=bare[1:],
                              over_bare_percent=100.0 * (stats[0] / bare[0] - 1.0), reduce_read_mb_per_episode=188.0 * N * EP / 1e6,
                              step_kernel=eng.last_step_kernel())))
        eng.close()


if __name__ == "__main__":
    main()
