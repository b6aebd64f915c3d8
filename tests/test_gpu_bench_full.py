"""A plain bench.py run does only what its headline needs; --full adds the measurements that take runs of their own, after
the timed region, without changing what the timed steps compute."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, EPISODE, WARMUP, STEPS = 256, 96, 4, 200
FULL_ONLY = ("episode_boundary", "rollout", "closed_loop", "secondary", "cpu_baseline")


def _bench(out_dir, *extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--envs-per-gpu", str(N), "--episode-steps", str(EPISODE), "--no-fill", "--dump-outputs", str(out_dir), *extra],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench(tmp_path / "plain")
    assert not set(FULL_ONLY) & set(plain), sorted(plain)
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["timed_steps"] == STEPS and plain["config"]["faults"] == 0
    assert not (plain["roofline"]["pmc_source"] or "").startswith("this run")       # no counter passes of its own
    full = _bench(tmp_path / "full", "--full", "--no-pmc", "--no-secondary", "--no-cpu-baseline")
    for k in ("episode_boundary", "rollout", "closed_loop"):
        assert k in full and "error" not in full[k], (k, full.get(k))
    assert full["rollout"]["value"] > 0 and full["closed_loop"]["value"] > 0
    assert full["episode_boundary"]["reset_plus_features_us"] > 0
    assert "secondary" not in full and "cpu_baseline" not in full
    # the extra legs run after the timed region: the same steps, the same episodes, the same outputs of the last timed step
    assert full["timed_steps"] == plain["timed_steps"] and full["return_stats"] == plain["return_stats"]
    for name in os.listdir(tmp_path / "plain"):
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name), err_msg=name)


def test_plain_run_at_the_headline_size_is_lean():
    """The headline workload (4096 envs, 10 000-step history fill) spends at most 30 s of a plain run's wall time, start to exit,
    outside its warm-up and timed steps."""
    steps, warmup = 200, 20
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    d = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert d["config"]["history_fill_steps"] == 10000 and d["timed_steps"] == steps
    assert wall - (steps + warmup) * d["ms_per_step"] * 1e-3 <= 30.0, wall
