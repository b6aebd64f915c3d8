#!/usr/bin/env python3
"""Generate tests/golden/onpolicy/onpolicy_returns.npz from the *imported* reference: the returns its OnPolicyCriticBufferEP.compute_returns
gives for T = 37 steps of N = 65 envs.  Nothing of the reference's sources is copied: the fixture holds the inputs (rewards, dones,
denormalised values, for one case the raw predictions and the ValueNorm's three tensors) and the reference's returns.

Cases: the three (gamma, gae_lambda) pairs of tests/onpolicy_ref.py x use_gae on / off, each over done flags at the first step, at the
last step, on consecutive steps and nowhere (columns of one batch) -- `plain`; and one case through a real ValueNorm (`norm`): raw
predictions go into the buffer, compute_returns denormalises them itself, and the fixture stores ValueNorm.denormalize of them as the
values.  use_proper_time_limits is run both ways and must agree (the reference sets bad_masks nowhere).

Needs the reference checkout: SDC_REFERENCE=<path> python tests/golden/gen_onpolicy_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
T, N = 37, 65


def _reference():
    ref = os.environ.get("SDC_REFERENCE")
    if not ref or not os.path.isdir(ref):
        sys.exit("set SDC_REFERENCE to the reference checkout")
    for p in (ref, os.path.join(HERE, "_shims"), os.path.join(REPO, "tests", "aux", "harl_stubs")):
        sys.path.insert(0, p)
    sys.path.insert(0, REPO)
    from harl.common.buffers.on_policy_critic_buffer_ep import OnPolicyCriticBufferEP
    from harl.common.valuenorm import ValueNorm
    return OnPolicyCriticBufferEP, ValueNorm


def _dones():
    """[T, N] uint8: env n % 4 == 0 never done, 1 at the first step, 2 at the last, 3 on two consecutive steps (which ones moves with n)"""
    d = np.zeros((T, N), dtype=np.uint8)
    for n in range(N):
        k = n % 4
        if k == 1:
            d[0, n] = 1
        elif k == 2:
            d[T - 1, n] = 1
        elif k == 3:
            t = 1 + (n * 7) % (T - 3)
            d[t, n] = d[t + 1, n] = 1
    return d


def _returns(Buffer, rew, done, preds, gamma, lam, use_gae, proper, normalizer=None):
    """the reference's returns [T, N] for predictions `preds` [T+1, N] (raw ones with a normalizer), filled through insert()"""
    args = dict(episode_length=T, n_rollout_threads=N, hidden_sizes=[64, 64], recurrent_n=1, gamma=gamma, gae_lambda=lam,
                use_gae=use_gae, use_proper_time_limits=proper)
    buf = Buffer(args, [29])
    rnn = np.zeros((N, 1, 64), dtype=np.float32)
    for t in range(T):
        masks = np.where(done[t] != 0, 0.0, 1.0).astype(np.float32)[:, None]
        buf.insert(np.zeros((N, 29), dtype=np.float32), rnn, preds[t][:, None], rew[t][:, None], masks, np.ones_like(masks))
    buf.compute_returns(preds[T][:, None], normalizer)
    assert buf.returns.dtype == np.float32
    return buf.returns[:T, :, 0].copy()


def main():
    Buffer, ValueNorm = _reference()
    from tests import onpolicy_ref as R
    import torch
    rng = np.random.default_rng(20260)
    rew = rng.standard_normal((T, N)).astype(np.float32)
    values = (rng.standard_normal((T + 1, N)) * 3.0).astype(np.float32)
    done = _dones()
    out = dict(rew=rew, done=done, values=values, gamma_lambda=np.asarray(R.GAMMA_LAMBDA, dtype=np.float64))
    for i, (gamma, lam) in enumerate(R.GAMMA_LAMBDA):
        for use_gae in (0, 1):
            a = _returns(Buffer, rew, done, values, gamma, lam, bool(use_gae), False)
            b = _returns(Buffer, rew, done, values, gamma, lam, bool(use_gae), True)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "use_proper_time_limits changed the returns"
            out[f"plain_returns_{i}_{use_gae}"] = a
    # one case through a real ValueNorm after a few updates
    vn = ValueNorm(1)
    for k in range(5):
        vn.update(torch.from_numpy((rng.standard_normal((64, 1)) * 4.0 - 2.5).astype(np.float32)))
    raw = rng.standard_normal((T + 1, N)).astype(np.float32)
    denorm = vn.denormalize(raw[..., None])[..., 0]
    assert denorm.dtype == np.float32 and denorm.shape == (T + 1, N)
    gamma, lam = R.GAMMA_LAMBDA[0]
    out.update(norm_raw=raw, norm_values=denorm, norm_running_mean=vn.running_mean.numpy().copy(),
               norm_running_mean_sq=vn.running_mean_sq.numpy().copy(), norm_debiasing_term=vn.debiasing_term.numpy().copy(),
               norm_returns=_returns(Buffer, rew, done, raw, gamma, lam, True, True, vn))
    os.makedirs(os.path.join(HERE, "onpolicy"), exist_ok=True)
    path = os.path.join(HERE, "onpolicy", "onpolicy_returns.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
