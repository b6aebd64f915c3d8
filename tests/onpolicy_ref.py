"""The on-policy batch restated in NumPy (include/sustaindc_hip.h THE ON-POLICY BATCH): sdc_gae's recurrence, masks, value predictions
and moments, and sdc_action_log_probs' fp64 log-probability and entropy rounded once to fp32.  One NumPy operation per operation of
the header, every operand an fp32 array or an np.float32 scalar, so that nothing is promoted or fused: tests/test_onpolicy_ref.py holds
`gae` to the reference's OnPolicyCriticBufferEP.compute_returns bit for bit (tests/golden/onpolicy/onpolicy_returns.npz), and
tests/test_gpu_onpolicy.py holds the kernels to these functions.  A plain module: no GPU, no torch."""
import numpy as np

GAMMA_LAMBDA = ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0))      # the (gamma, gae_lambda) pairs every test runs
NAN_BITS = 0x7FC0DEAD                                      # the guard rows' fp32 pattern (a quiet NaN with a payload)
MOMENTS_BLOCK = 256                                        # csrc/sdc_onpolicy.hpp SDC_MOMENTS_BLOCK


def masks(done, first_done=None):
    """done [T, N] uint8, first_done [N] uint8 or None -> masks [T+1, N] fp32"""
    T, N = done.shape
    m = np.ones((T + 1, N), dtype=np.float32)
    if first_done is not None:
        m[0] = np.where(np.asarray(first_done) != 0, np.float32(0), np.float32(1))
    m[1:] = np.where(np.asarray(done) != 0, np.float32(0), np.float32(1))
    return m


def gae(rew, done, values, gamma, gae_lambda, use_gae=True, reward_agent=0, first_done=None):
    """rew [T, N, 3] fp32, done [T, N] uint8, values [T+1, N] fp32 -> (returns [T, N], advantages [T, N], masks [T+1, N]), fp32"""
    rew, values = np.asarray(rew), np.asarray(values)
    assert rew.dtype == np.float32 and values.dtype == np.float32
    T, N = done.shape
    assert rew.shape == (T, N, 3) and values.shape == (T + 1, N)
    g = np.float32(gamma)
    c = np.float32(float(gamma) * float(gae_lambda))      # the product in double, rounded once
    M = masks(done, first_done)
    r = np.ascontiguousarray(rew[:, :, reward_agent])
    returns = np.empty((T, N), dtype=np.float32)
    run = np.zeros(N, dtype=np.float32) if use_gae else values[T].copy()
    for t in range(T - 1, -1, -1):
        m = M[t + 1]
        if use_gae:
            delta = (r[t] + (g * values[t + 1]) * m) - values[t]
            run = delta + (c * m) * run
            returns[t] = run + values[t]
        else:
            run = (run * g) * m + r[t]
            returns[t] = run
    advantages = returns - values[:T]
    assert returns.dtype == advantages.dtype == np.float32
    return returns, advantages, M


def value_preds(values, scale, shift):
    """(V - shift) / scale in fp32"""
    return (np.asarray(values, dtype=np.float32) - np.float32(shift)) / np.float32(scale)


def moments(advantages):
    """[T, N] fp32 -> (mean, population standard deviation) in fp64 in the kernels' order: per env the walk t = T-1 .. 0, then the envs
    l, l + 256, ... of partial l, then the halving tree"""
    a = np.asarray(advantages, dtype=np.float32).astype(np.float64)
    T, N = a.shape
    s1, s2 = np.zeros(N), np.zeros(N)
    for t in range(T - 1, -1, -1):
        s1 = s1 + a[t]
        s2 = s2 + a[t] * a[t]
    part = np.zeros((MOMENTS_BLOCK, 2))
    for n in range(N):
        part[n % MOMENTS_BLOCK, 0] += s1[n]
        part[n % MOMENTS_BLOCK, 1] += s2[n]
    half = MOMENTS_BLOCK // 2
    while half >= 1:
        part[:half] = part[:half] + part[half:2 * half]
        half //= 2
    count = float(T) * float(N)
    mean = part[0, 0] / count
    var = part[0, 1] / count - mean * mean
    return mean, float(np.sqrt(max(var, 0.0)))


def action_log_probs(actions, logits, dtype=np.float64):
    """actions [..., 3] int, logits [..., 3, 3] fp32 -> (log_probs, entropy) [..., 3] fp32: the header's arithmetic in `dtype` (fp64;
    np.longdouble measures what fp64 itself loses), each result rounded once to fp32"""
    l = np.asarray(logits)
    assert l.dtype == np.float32
    m = l.max(-1, keepdims=True)                                    # in fp32
    z = l.astype(dtype) - m.astype(dtype)
    e = np.exp(z)
    s = (e[..., 0] + e[..., 1]) + e[..., 2]
    lp = z - np.log(s)[..., None]
    p = e / s[..., None]
    j = np.clip(np.asarray(actions), None, 2)
    j = np.where(j < 0, 2, j)                                        # (an action outside 0 .. 2 is read as 2)
    lpj = np.take_along_axis(lp, j[..., None].astype(np.int64), -1)[..., 0]
    ent = -((p[..., 0] * lp[..., 0] + p[..., 1] * lp[..., 1]) + p[..., 2] * lp[..., 2])
    return lpj.astype(np.float32), ent.astype(np.float32)


def ulps(a, b):
    """the distance of two fp32 arrays in units in the last place (of finite values of one sign, or equal ones)"""
    ia = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 31) - ib, ib)
    return np.abs(ia - ib)


# ---- the cases of the fixture and of the GPU tests -----------------------------------------------------------------------------------
DONE_PATTERNS = ("none", "staggered", "first", "last", "consecutive", "all")


def done_pattern(name, T, N):
    """[T, N] uint8: none; every env at a different step (env n at step n % T); the first step; the last step; two consecutive steps
    (T // 2 and the one behind it, where there is one); all at once (every env, at step T // 2)"""
    d = np.zeros((T, N), dtype=np.uint8)
    n = np.arange(N)
    if name == "staggered":
        d[n % T, n] = 1
    elif name == "first":
        d[0, n[::2]] = 1
    elif name == "last":
        d[T - 1, n[::2]] = 1
    elif name == "consecutive":
        d[T // 2, n[::2]] = 1
        d[min(T // 2 + 1, T - 1), n[::2]] = 1
    elif name == "all":
        d[T // 2, :] = 1
    else:
        assert name == "none"
    return d


def inputs(T, N, seed, magnitude=1.0):
    """(rew [T, N, 3], values [T+1, N]) fp32: rewards of order one, values of order `magnitude`"""
    rng = np.random.default_rng(seed)
    rew = rng.standard_normal((T, N, 3)).astype(np.float32)
    values = (rng.standard_normal((T + 1, N)) * magnitude).astype(np.float32)
    return rew, values
