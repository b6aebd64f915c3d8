"""Tests-only NumPy restatement of include/sustaindc_hip.h TRAIN ON THE DEVICE (TEST INFRASTRUCTURE, never imported by the product):
the keyed permutation over tests/reset_ref.philox4x32_10 and ValueNorm's running update, operation for operation -- Python ints for the
Feistel network, np.float32 per fp32 operation, Python floats (fp64) for the sums in the device's fixed two-stage order."""
from __future__ import annotations

import functools
import os

import numpy as np

from tests import reset_ref as RR

ROUNDS = 6
BLOCK, MAX_BLOCKS = 256, 1024
f32 = np.float32


def half_bits(n: int) -> int:
    """b: bits = bit length of (n - 1) (0 for n = 1); b = max(1, (bits + 1) // 2)"""
    return max(1, ((n - 1).bit_length() + 1) // 2)


def permutations(n: int, seed: int, stream_ids, rounds: int = ROUNDS):
    """perm [S, n] int32 for the S stream ids, and how many passes through the network the slowest index took.  Vectorised cycle
    walking: every pass sends the indices still at or above n through the network once more."""
    b = half_bits(n)
    mask = np.uint64((1 << b) - 1)
    streams = np.asarray(stream_ids, dtype=np.uint64).reshape(-1)
    k_lo, k_hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    x = np.broadcast_to(np.arange(n, dtype=np.uint64), (streams.size, n)).copy()
    s_lo = np.broadcast_to((streams & np.uint64(0xFFFFFFFF))[:, None], x.shape)
    s_hi = np.broadcast_to((streams >> np.uint64(32))[:, None], x.shape)
    todo = np.ones(x.shape, dtype=bool)
    passes = 0
    while todo.any():
        v, lo, hi = x[todo], s_lo[todo], s_hi[todo]
        L, R = v >> np.uint64(b), v & mask
        for r in range(rounds):
            F = RR.philox4x32_10(R, r, lo, hi, k_lo, k_hi)[0].astype(np.uint64) & mask
            L, R = R, L ^ F
        v = (L << np.uint64(b)) | R
        x[todo] = v
        todo[todo] = v >= n
        passes += 1
    return x.astype(np.int32), passes


def permutation(n: int, seed: int, stream_id: int = 0, rounds: int = ROUNDS):
    """perm [n] int32 of one stream, and the passes"""
    p, passes = permutations(n, seed, [stream_id], rounds)
    return p[0], passes


def blocks(n: int) -> int:
    return min((n + BLOCK - 1) // BLOCK, MAX_BLOCKS)


def _tree(p):
    """[2, 256] fp64 halved from 128 down: lane l < half takes lane l + half"""
    p = p.copy()
    half = BLOCK // 2
    while half >= 1:
        p[:, :half] = p[:, :half] + p[:, half:2 * half]
        half //= 2
    return p[:, 0]


def two_stage_sums(x):
    """(S1, S2) of fp32 values x in sdc_ppo_terms' order: S1 = sum (double)x, S2 = sum (double)(float)(x * x)"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    n, B = x.size, blocks(x.size)
    sq = (x * x).astype(np.float32)
    vals = np.stack([x.astype(np.float64), sq.astype(np.float64)])      # [2, n]
    stride = B * BLOCK
    passes = (n + stride - 1) // stride
    pad = np.zeros((2, passes * stride))
    pad[:, :n] = vals
    pad = pad.reshape(2, passes, B, BLOCK)
    live = (np.arange(passes * stride) < n).reshape(passes, B, BLOCK)
    lane = np.zeros((2, B, BLOCK))
    for k in range(passes):      # (s = s + x in rising k; an element past n is not added at all: -0.0 + 0.0 would not matter, NaN would)
        lane = np.where(live[k][None], lane + pad[:, k], lane)
    part = np.stack([_tree(lane[:, b]) for b in range(B)], axis=1)      # [2, B]
    fold = np.zeros((2, BLOCK))
    for b in range(B):
        fold[:, b % BLOCK] = fold[:, b % BLOCK] + part[:, b]
    s = _tree(fold)
    return float(s[0]), float(s[1])


def derive(rm, rsq, deb):
    """(scale, shift) of the three running values, fp32: dc_rl_amd.engine.value_norm_scale_shift's lines"""
    deb = np.maximum(f32(deb), f32(1e-5))
    mean, mean_sq = f32(f32(rm) / deb), f32(f32(rsq) / deb)
    var = np.maximum(f32(mean_sq - f32(mean * mean)), f32(1e-2))
    return f32(np.sqrt(var)), mean


def value_norm_update(state, x, beta=0.99999):
    """state (running_mean, running_mean_sq, debiasing_term) as np.float32 -> the state after ValueNorm.update(x), and (scale, shift)"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    S1, S2 = two_stage_sums(x)
    n = float(x.size)
    bm, bsq = f32(S1 / n), f32(S2 / n)
    w, omw = f32(beta), f32(1.0 - beta)
    rm, rsq, deb = (f32(v) for v in state)
    rm = f32(f32(rm * w) + f32(bm * omw))
    rsq = f32(f32(rsq * w) + f32(bsq * omw))
    deb = f32(f32(deb * w) + omw)
    return (rm, rsq, deb), derive(rm, rsq, deb)


# ---- the fixture the reference wrote (tests/golden/train/train.npz, tests/golden/gen_train_golden.py) ---------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train", "train.npz")
MARGIN = 8.0      # the project's multiple of the reference's own fp32 distance from its fp64 run


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def derive64(rm, rsq, deb):
    """(scale, shift) of three fp64 running values, in fp64"""
    deb = max(float(deb), 1e-5)
    mean = float(rm) / deb
    return float(np.sqrt(max(float(rsq) / deb - mean * mean, 1e-2))), mean


def scale_shift_distance(mine, state64):
    """the larger relative distance of (scale, shift) `mine` from what the fp64 running values `state64` give"""
    scale, shift = derive64(*state64)
    return max(abs(float(mine[0]) - scale) / scale, abs(float(mine[1]) - shift) / abs(shift))


def position_value_counts(n, seed, streams, rounds=ROUNDS):
    """counts [n, n]: how often position i held value v over the streams 0 .. streams-1"""
    p = permutations(n, seed, np.arange(streams), rounds)[0]
    cnt = np.zeros((n, n), dtype=np.int64)
    np.add.at(cnt, (np.broadcast_to(np.arange(n), p.shape), p), 1)
    return cnt
