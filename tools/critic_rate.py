"""Measurement: the critic kernel (SdcEngine.critic_values: one launch of sdc_critic_values_kernel) against what a user runs without
it -- the same network as a torch fp32 module on the GPU, eager (three Linear, three LayerNorm, two activations, the ValueNorm's
multiply-add) -- on the row counts of one actor-stats chunk, [105, 4096, 29] and [12, 32768, 29], and of the planners' terminal case,
[4096, 29]; then plan_cem at 4 096 envs (horizon 8, 64 candidates, 3 iterations) with and without the critic as terminal value,
alternated.  ONE process; device events around each call, one warm-up, then the median, min and max of nine.  One JSON line per size,
with the achieved bytes/s (116 B read + 4 B written per row) and matrix-instruction FLOP/s (2 x (32 x 64 + 64 x 64) per row: the
padded first layer as issued) next to the fp32 matrix peak of 157.3 TF, and the largest difference between the two routes' values.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/critic_rate.py` for the kernels' own times."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from tools.mark_rate import timed3

REPS = 9
FP32_MATRIX_PEAK = 157.3e12
VALUE_NORM = (-3.0, 56.25)      # (mean, var)


def critic_weights(seed=11):
    """random weights of the reference's VNet shape (LayerNorm(29)-64-64-1, tanh), as the fields of sdc_critic_params"""
    r = np.random.default_rng(seed)
    return {"ln0_g": 1 + 0.1 * r.standard_normal(29), "ln0_b": 0.1 * r.standard_normal(29),
            "w1": r.standard_normal((64, 29)) * 0.3, "b1": 0.1 * r.standard_normal(64),
            "ln1_g": 1 + 0.1 * r.standard_normal(64), "ln1_b": 0.1 * r.standard_normal(64),
            "w2": r.standard_normal((64, 64)) * 0.2, "b2": 0.1 * r.standard_normal(64),
            "ln2_g": 1 + 0.1 * r.standard_normal(64), "ln2_b": 0.1 * r.standard_normal(64),
            "w3": r.standard_normal(64) * 0.2, "b3": np.zeros(())}


class TorchCritic(torch.nn.Module):
    def __init__(self, w, value_norm):
        super().__init__()
        nn = torch.nn
        self.norm = nn.LayerNorm(29)
        self.fc = nn.Sequential(nn.Linear(29, 64), nn.Tanh(), nn.LayerNorm(64), nn.Linear(64, 64), nn.Tanh(), nn.LayerNorm(64))
        self.v_out = nn.Linear(64, 1)
        self.scale, self.shift = float(np.sqrt(value_norm[1])), float(value_norm[0])
        put = lambda p, a: p.data.copy_(torch.as_tensor(np.asarray(a, dtype=np.float32)).reshape(p.shape))
        put(self.norm.weight, w["ln0_g"]); put(self.norm.bias, w["ln0_b"])
        put(self.fc[0].weight, w["w1"]); put(self.fc[0].bias, w["b1"]); put(self.fc[2].weight, w["ln1_g"]); put(self.fc[2].bias, w["ln1_b"])
        put(self.fc[3].weight, w["w2"]); put(self.fc[3].bias, w["b2"]); put(self.fc[5].weight, w["ln2_g"]); put(self.fc[5].bias, w["ln2_b"])
        put(self.v_out.weight, w["w3"]); put(self.v_out.bias, w["b3"])

    @torch.no_grad()
    def forward(self, x):
        return self.v_out(self.fc(self.norm(x)))[..., 0] * self.scale + self.shift


def main():
    N = 4096
    eng, _, _ = bench.build_engine(N, 96, 0, seed=99, debug_flags=0)
    w = critic_weights()
    eng.set_critic(w, VALUE_NORM, "tanh")
    module = TorchCritic(w, VALUE_NORM).to(eng.device)
    g = torch.Generator().manual_seed(5)
    for shape in ((105, 4096, 29), (12, 32768, 29), (4096, 29)):
        x = torch.randn(shape, generator=g).to(eng.device)
        rows = x.numel() // 29
        diff = float((eng.critic_values(x) - module(x)).abs().max())      # (warm: both routes have run once)
        torch.cuda.synchronize()
        kernel = timed3(lambda: eng.critic_values(x), REPS)
        eager = timed3(lambda: module(x), REPS)
        print(json.dumps(dict(what="critic_values", shape=list(shape), rows=rows, kernel_ms=kernel[0], kernel_ms_range=kernel[1:],
                              torch_eager_ms=eager[0], torch_eager_ms_range=eager[1:], speedup=eager[0] / kernel[0],
                              kernel_GBps=rows * 120.0 / kernel[0] / 1e6, kernel_matrix_TFLOPs=rows * 2.0 * (32 * 64 + 64 * 64) / kernel[0] / 1e9,
                              share_of_fp32_matrix_peak=rows * 2.0 * (32 * 64 + 64 * 64) / (kernel[0] * 1e-3) / FP32_MATRIX_PEAK,
                              max_abs_difference=diff, kernel_name=eng.last_step_kernel())), flush=True)
    # the planners' terminal value: plan_cem with and without it, alternated
    eng.reset()
    K, M, IT = 8, 64, 3
    plan = lambda: eng.plan_cem(K, IT, M, 8, seed=1, draw=0)
    times = {0.0: [], 0.5: []}
    for weight in (0.0, 0.5):
        eng.set_plan_critic(weight)
        plan()                                                                # (warm: the handle's buffers are allocated)
    torch.cuda.synchronize()
    for _ in range(REPS):
        for weight in (0.0, 0.5):
            eng.set_plan_critic(weight)
            times[weight].append(timed3(plan, 1)[0])
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps(dict(what="plan_cem", n_envs=N, horizon=K, candidates=M, iterations=IT, without_ms=med[0.0],
                          without_ms_range=[min(times[0.0]), max(times[0.0])], with_ms=med[0.5],
                          with_ms_range=[min(times[0.5]), max(times[0.5])], added_ms_per_call=med[0.5] - med[0.0],
                          added_us_per_candidate=(med[0.5] - med[0.0]) * 1e3 / (M * IT), last_kernel=eng.last_step_kernel())), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
