"""tests/optim_ref.py (the NumPy restatement of include/sustaindc_hip.h THE OPTIMISER STEP) against torch.optim.Adam(foreach=False,
fused=False) behind clip_grad_norm_ on the CPU: 10 steps over gradients that span 1e-8 .. 1e3 with exact zeros, weight decay 0 and 0.01,
clipping active, inactive and off.  torch fp64 is the truth: the restatement's largest distance to it, in units of lr, may be at most 4
times torch fp32's own distance on the same inputs -- both are elementwise fp32 chains of equal length; the factor leaves room for the
three pre-rounded scalars and the lerp form.  DESIGN.md section 4.31 records the distances this prints.  And the exact cases."""
import numpy as np
import pytest

from tests import optim_ref as O

N, STEPS, LR, BETAS, EPS = 6391, 10, 5e-4, (0.9, 0.999), 1e-5
CLIPS = {"active": 10.0, "inactive": 1e6, "off": None}


def inputs(seed=11):
    rng = np.random.default_rng(seed)
    p0 = (rng.standard_normal(N) * 0.3).astype(np.float32)
    grads = []
    for _ in range(STEPS):
        g = (10.0 ** rng.uniform(-8, 3, N)) * rng.choice([-1.0, 1.0], N)
        g[rng.random(N) < 0.1] = 0.0
        grads.append(g.astype(np.float32))
    return p0, grads


def ref_run(p0, grads, wd, clip, first=0):
    p, m, v, st = p0.copy(), np.zeros(N, np.float32), np.zeros(N, np.float32), O.new_state()
    out = []
    for g in grads:
        p, m, v, _ = O.step(g, p, m, v, st, LR, BETAS, EPS, wd, clip, first=first)
        out.append(p.astype(np.float64))
    return out, st


@pytest.mark.parametrize("clip", sorted(CLIPS))
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_restatement_within_4x_of_torch_fp32(wd, clip):
    import torch
    p0, grads = inputs()
    truth = O.torch_run(grads, p0, torch.float64, LR, BETAS, EPS, wd, CLIPS[clip])
    t32 = O.torch_run(grads, p0, torch.float32, LR, BETAS, EPS, wd, CLIPS[clip])
    ref, st = ref_run(p0, grads, wd, CLIPS[clip])
    assert st == dict(step=STEPS, beta1_pow=pytest.approx(0.9 ** STEPS, rel=1e-14), beta2_pow=pytest.approx(0.999 ** STEPS, rel=1e-14), skipped=0)
    d_ref = max(float(np.abs(a - b).max()) for a, b in zip(ref, truth)) / LR
    d_t32 = max(float(np.abs(a - b).max()) for a, b in zip(t32, truth)) / LR
    a32, b32 = ref[-1].astype(np.float32), t32[-1].astype(np.float32)
    ulps = np.abs(a32.view(np.int32).astype(np.int64) - b32.view(np.int32).astype(np.int64))
    print("wd %g clip %s: restatement %.3e lr, torch fp32 %.3e lr from torch fp64; restatement vs torch fp32 after %d steps: max %d ulp, "
          "%d of %d elements differ" % (wd, clip, d_ref, d_t32, STEPS, int(ulps.max()), int((ulps != 0).sum()), N))
    assert d_t32 > 0.0
    assert d_ref <= 4.0 * d_t32


def test_zero_gradient_on_zero_moments_leaves_p():
    p0, _ = inputs()
    z = np.zeros(N, np.float32)
    st = O.new_state()
    p, m, v, norm = O.step(z, p0, z, z, st, LR, BETAS, EPS, 0.0, 10.0)
    assert norm == 0.0 and st["step"] == 1 and st["skipped"] == 0
    assert p.tobytes() == p0.tobytes() and not m.any() and not v.any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_gradient_changes_nothing_but_skipped(bad):
    p0, grads = inputs()
    p, m, v, st = p0.copy(), np.zeros(N, np.float32), np.zeros(N, np.float32), O.new_state()
    p, m, v, _ = O.step(grads[0], p, m, v, st, LR, BETAS, EPS, 0.01, 10.0)
    before = dict(st)
    g = grads[1].copy()
    g[4321] = bad
    p2, m2, v2, norm = O.step(g, p, m, v, st, LR, BETAS, EPS, 0.01, 10.0)
    assert not np.isfinite(norm)
    assert (p2.tobytes(), m2.tobytes(), v2.tobytes()) == (p.tobytes(), m.tobytes(), v.tobytes())
    assert st == dict(before, skipped=1)
    # the next clean step is the step that would have followed the first
    st_b = dict(before)
    want = O.step(grads[2], p, m, v, st_b, LR, BETAS, EPS, 0.01, 10.0)
    got = O.step(grads[2], p2, m2, v2, st, LR, BETAS, EPS, 0.01, 10.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want[:3], got[:3])) and st == dict(st_b, skipped=1)


def test_ln0_untouched_with_feature_norm_off_and_weight_decay_on():
    p0, grads = inputs()
    first = 52
    g = grads[0].copy()
    g[:first] = 0.0          # (exact zeros by the backward's contract)
    z = np.zeros(N, np.float32)
    p, m, v, _ = O.step(g, p0, z, z, O.new_state(), LR, BETAS, EPS, 0.01, 10.0, first=first)
    assert p[:first].tobytes() == p0[:first].tobytes() and not m[:first].any() and not v[:first].any()
    assert (p[first:] != p0[first:]).mean() > 0.9
    # ... where a step over them would have moved them by the weight decay
    q, _, _, _ = O.step(g, p0, z, z, O.new_state(), LR, BETAS, EPS, 0.01, 10.0, first=0)
    assert (q[:first] != p0[:first]).any()
