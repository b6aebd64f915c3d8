"""Measurement: one 672-step episode of 4 096 and of 32 768 envs played by the three in-kernel actors (sampled), three ways in ONE process --
  rollout_actor_stats   SdcEngine.rollout_actor_stats (one sdc_rollout_actor_stats call: closed-loop rollouts into the handle's output
                        block in chunks, one launch of sdc_stats_reduce_kernel and one of sdc_policy_stats_kernel per chunk);
  python_loop           the route it replaces: a Python loop of `rollout_actor` chunks of the same length, each chunk's info and rew
                        reduced with torch.sum / amin / amax and a count of positive values, its actions and logits with log_softmax,
                        gather and comparisons, into fp64 accumulators;
  bare_rollouts         sdc_rollout_actor calls of the same chunks into a preallocated block, nothing reduced: the floor.
Device events around each episode, one warm-up episode each, then the median, min and max of nine.  Every episode starts at an episode's
first step (the auto-reset of the one before).  One JSON line per size, with the chunk length and the bytes the two reduce kernels read
per episode (188 and 48 B per env-step).  Run it under `rocprofv3 --kernel-trace --stats -- python tools/policy_eval_rate.py` for the
kernels' own times."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from dc_rl_amd import _lib as L
from tools.clone_rate import EP
from tools.eval_rate import chunk_steps
from tools.mark_rate import timed3

REPS = 9


def python_loop(eng, chunk):
    N, dev = eng.n_envs, eng.device
    f64 = dict(dtype=torch.float64, device=dev)
    s, npos = torch.zeros((N, L.INFO_DIM), **f64), torch.zeros((N, L.INFO_DIM), **f64)
    lo = torch.full((N, L.INFO_DIM), float("inf"), dtype=torch.float32, device=dev)
    hi = torch.full((N, L.INFO_DIM), float("-inf"), dtype=torch.float32, device=dev)
    ret = torch.zeros((N, 3), **f64)
    n = torch.zeros((N, 3, 3), dtype=torch.int64, device=dev)
    sw = torch.zeros((N, 3), dtype=torch.int64, device=dev)
    logp, ent = torch.zeros((N, 3), **f64), torch.zeros((N, 3), **f64)
    which = torch.arange(3, dtype=torch.int32, device=dev)
    last = None
    for k0 in range(0, EP, chunk):
        o = eng.rollout_actor(min(chunk, EP - k0), sample=True, want_logits=True)
        rew, info, acts, logits = o[2], o[4], o[5], o[6]
        s += info.sum(0, dtype=torch.float64)
        lo = torch.minimum(lo, info.amin(0))
        hi = torch.maximum(hi, info.amax(0))
        npos += (info > 0).sum(0)
        ret += rew.sum(0, dtype=torch.float64)
        n += (acts[..., None] == which).sum(0)
        sw += (acts[1:] != acts[:-1]).sum(0)
        if last is not None:
            sw += acts[0] != last
        last = acts[-1]
        lp = torch.log_softmax(logits.double(), -1)
        logp += torch.gather(lp, -1, acts.long()[..., None])[..., 0].sum(0)
        ent -= (lp.exp() * lp).sum(-1).sum(0)
    return s, lo, hi, npos, ret, n, sw, logp, ent


def bare_rollouts(eng, chunk, block):
    p = lambda x: C.c_void_p(x.data_ptr())
    for k0 in range(0, EP, chunk):
        L.check(eng.lib.sdc_rollout_actor(eng._h, min(chunk, EP - k0), 1, p(block["obs"]), p(block["share"]), p(block["rew"]), p(block["done"]),
                                          p(block["info"]), p(eng.final_obs), p(block["acts"]), p(block["logits"]), eng._stream()))


def main():
    for N in (4096, 32768):
        eng, _, _ = bench.build_engine(N, EP, 0, seed=99, debug_flags=0)
        for a, w in enumerate(bench.actor_weights()):
            eng.set_actor(a, w)
        eng.reset()
        chunk = chunk_steps(N, EP)
        kw = dict(dtype=torch.float32, device=eng.device)
        block = dict(obs=torch.empty((chunk, N, L.N_AGENTS, L.OBS_PAD), **kw), share=torch.empty((chunk, N, L.SHARE_OBS_DIM), **kw),
                     rew=torch.empty((chunk, N, L.N_AGENTS), **kw), info=torch.empty((chunk, N, L.INFO_DIM), **kw),
                     done=torch.empty((chunk, N), dtype=torch.uint8, device=eng.device),
                     acts=torch.empty((chunk, N, 3), dtype=torch.int32, device=eng.device), logits=torch.empty((chunk, N, 3, 3), **kw))
        st = eng.rollout_actor_stats(EP, sample=True)      # (warm: the handle's buffers are allocated; every route runs one episode)
        python_loop(eng, chunk)
        bare_rollouts(eng, chunk, block)
        torch.cuda.synchronize()
        assert eng.steps_to_episode_end() == EP and int(st.steps.min()) == EP and int(st.policy.action_counts.sum(-1).min()) == EP
        stats = timed3(lambda: eng.rollout_actor_stats(EP, sample=True), REPS)
        loop = timed3(lambda: python_loop(eng, chunk), REPS)
        bare = timed3(lambda: bare_rollouts(eng, chunk, block), REPS)
        print(json.dumps(dict(what="rollout_actor_stats", n_envs=N, episode_steps=EP, chunk_steps=chunk, chunks=-(-EP // chunk),
                              rollout_actor_stats_ms=stats[0], rollout_actor_stats_ms_range=stats[1:], python_loop_ms=loop[0],
                              python_loop_ms_range=loop[1:], bare_rollouts_ms=bare[0], bare_rollouts_ms_range=bare[1:],
                              over_bare_percent=100.0 * (stats[0] / bare[0] - 1.0), reduce_read_mb_per_episode=188.0 * N * EP / 1e6,
                              policy_read_mb_per_episode=48.0 * N * EP / 1e6, step_kernel=eng.last_step_kernel())), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
