"""sdc_ppo_terms restated in NumPy (include/sustaindc_hip.h EVALUATE THE ACTORS ON STORED ROWS): the per-element arithmetic in fp64, one
NumPy operation per operation of the header and each stored value rounded once to fp32; and the two-stage summation order of `stats`.
tests/test_ppo_ref.py holds `terms` to what the reference's HAPPO.update returned (tests/golden/actor_eval/actor_eval.npz),
tests/test_gpu_actor_eval.py holds the kernels to these functions.  A plain module: no GPU, no torch."""
import numpy as np

BLOCK = 256             # csrc/sdc_actor_eval.hpp SDC_PPO_BLOCK
MAX_BLOCKS = 1024       # csrc/sdc_actor_eval.hpp SDC_PPO_MAX_BLOCKS
EDGE = 1e-12            # |r / edge - 1| <= EDGE: which side of a clip edge r lies on is not sure (the device's exp is its own library's);
                        # lr = 0 is sure on every side: exp(0) is exactly 1 in any exp


def blocks(n):
    """stage 1's workgroups for n = T N elements"""
    return min((n + BLOCK - 1) // BLOCK, MAX_BLOCKS)


def terms(new_log_probs, old_log_probs, advantages, agent, clip_param, factor=None, dtype=np.float64):
    """new_log_probs, old_log_probs [..., 3] fp32 (column `agent` is read), advantages and factor (or None) [...] fp32 -> a dict of
    ratio, surr, factor_out (fp32), lr and r (`dtype`), clipped and unsure (bool), all [...]: the header's arithmetic in `dtype`
    (fp64; np.longdouble measures what fp64 itself loses)"""
    new, old, adv = np.asarray(new_log_probs), np.asarray(old_log_probs), np.asarray(advantages)
    assert new.dtype == old.dtype == adv.dtype == np.float32
    lr = new[..., agent].astype(dtype) - old[..., agent].astype(dtype)
    r = np.exp(lr)
    ratio = r.astype(np.float32)
    A = adv.astype(dtype)
    f32 = np.ones(adv.shape, dtype=np.float32) if factor is None else np.asarray(factor)
    assert f32.dtype == np.float32
    F = f32.astype(dtype)
    lo, hi = dtype(1.0 - float(clip_param)), dtype(1.0 + float(clip_param))      # (1 -+ clip in double, as the library forms them)
    s1 = r * A
    rc = np.where(r < lo, lo, r)
    rc = np.where(rc > hi, hi, rc)
    s2 = rc * A
    m = np.where(s2 < s1, s2, s1)
    surr = (F * m).astype(np.float32)
    factor_out = f32 * ratio                                                      # one fp32 product of the stored values
    assert factor_out.dtype == np.float32
    clipped = (r < lo) | (r > hi)
    unsure = (lr != 0) & ((np.abs(r / lo - 1.0) <= EDGE) | (np.abs(r / hi - 1.0) <= EDGE))
    return dict(ratio=ratio, surr=surr, factor_out=factor_out, lr=lr.astype(np.float64), r=r, clipped=clipped, unsure=unsure)


def _halve(part, take):
    """[..., 256] -> [...]: entry l takes entry l + half, half = 128 .. 1"""
    part = part.copy()
    half = BLOCK // 2
    while half >= 1:
        part[..., :half] = take(part[..., :half], part[..., half:2 * half])
        half //= 2
    return part[..., 0]


def ordered(x, kind):
    """the fp64 values x (flat, element order) folded in the kernels' order; kind "sum", "min" or "max" -> one fp64 value"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    start, take = {"sum": (0.0, lambda a, b: a + b), "min": (np.inf, lambda a, b: np.where(b < a, b, a)),
                   "max": (-np.inf, lambda a, b: np.where(b > a, b, a))}[kind]
    n = x.size
    B = blocks(n)
    # stage 1: lane l of workgroup b folds elements b * 256 + l + k * 256 * B, k = 0, 1, ...; a missing element leaves the lane as it is
    K = (n + B * BLOCK - 1) // (B * BLOCK)
    pad = np.full(K * B * BLOCK, start)
    pad[:n] = x
    pad = pad.reshape(K, B, BLOCK)
    acc = np.full((B, BLOCK), start)
    for k in range(K):
        acc = take(acc, pad[k])
    part = _halve(acc, take)                                                      # [B]
    # stage 2: lane l folds partials l, l + 256, ...
    K2 = (B + BLOCK - 1) // BLOCK
    pad = np.full(K2 * BLOCK, start)
    pad[:B] = part
    pad = pad.reshape(K2, BLOCK)
    acc = np.full(BLOCK, start)
    for k in range(K2):
        acc = take(acc, pad[k])
    return float(_halve(acc, take))


def stats(surr, ratio, lr, entropy_col, clipped):
    """the eight statistics from the STORED fp32 surr and ratio, lr (fp64, exact), the agent's fp32 entropy column (or None) and the
    clipped flags, all [...]: fp64 [8] in the kernels' order"""
    surr, ratio = np.asarray(surr), np.asarray(ratio)
    assert surr.dtype == ratio.dtype == np.float32
    rd = ratio.astype(np.float64)
    ent = 0.0 if entropy_col is None else ordered(np.asarray(entropy_col, dtype=np.float32).astype(np.float64), "sum")
    return np.array([ordered(surr.astype(np.float64), "sum"), ordered(rd, "sum"), ordered(lr, "sum"), ent,
                     ordered(np.asarray(clipped).astype(np.float64), "sum"), ordered(rd, "min"), ordered(rd, "max"), float(ratio.size)])


def summary(s):
    """PPOTerms.summary from stats [8]"""
    n = float(s[7])
    return dict(policy_loss=-float(s[0]) / n, ratio_mean=float(s[1]) / n, ratio_min=float(s[5]), ratio_max=float(s[6]),
                approx_kl=-float(s[2]) / n, entropy=float(s[3]) / n, clip_frac=float(s[4]) / n)


def ulps(a, b):
    """the distance of two fp32 arrays in units in the last place (tests/onpolicy_ref.ulps)"""
    from tests.onpolicy_ref import ulps as u
    return u(a, b)

