"""The decision schedule of sdc_rollout_cem_stats (csrc/sdc_mpc_schedule.hpp) without a GPU: the header compiled by g++ alone into a
program that reads calls and prints every step's decision, held to a restatement in Python of what the agent does (agents._mpc_horizon
and CEMMPCAgent._start / act, as a state machine over the carried result's length and the step of the decision before), and the same
program built with -fsanitize=address,undefined, run over the same input.

A request line:  horizon warm_start auto_reset resume_steps left n_steps   (resume_steps 0: no resume)
The answer: per step  K planned fresh draw_index,  then the number of planned decisions by the schedule and by sdc_mpc_planned."""
import subprocess

import pytest

from dc_rl_amd import _lib as L

EP = 12
DRIVER = r"""
#include <cstdio>
#include "sdc_mpc_schedule.hpp"
int main() {
  int H, warm, auto_reset, resume_steps, left, n_steps;
  while (std::scanf("%d %d %d %d %d %d", &H, &warm, &auto_reset, &resume_steps, &left, &n_steps) == 6) {
    SdcMpcSchedule S(H, warm, auto_reset, resume_steps);
    for (int t = 0; t < n_steps; t++) {
      const SdcMpcDecision d = S.next(left - t);
      std::printf("%d %d %d %u ", d.steps, d.planned, d.fresh, d.draw_index);
    }
    std::printf("| %u %u\n", S.planned, sdc_mpc_planned(H, auto_reset, left, n_steps));
  }
  return 0;
}
"""


def _build(tmp_path, name, extra):
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + L.CSRC] + extra + [str(src), "-o", exe], check=True)
    return exe


def _agent(H, warm, auto_reset, resume_steps, left, n_steps):
    """n_steps rounds of CEMMPCAgent.act + a step, restated: the agent's state is the length of the result it carries (None: nothing),
    the episode step of its last decision and its draw counter.  A resumed call is an agent that decided one step earlier."""
    start = EP - left
    carried = resume_steps if resume_steps else None
    prev = start - 1 if resume_steps else None
    draw, out = 0, []
    for step in range(start, start + n_steps):
        lt = EP - step
        K = min(H, lt - 1 if auto_reset else lt)                      # _mpc_horizon
        K = K if lt >= 2 and K >= 1 else 0
        if K == 0:                                                    # act: the do-nothing fallback
            carried, prev = None, step
            out.append((0, 0, 0, 0))
            continue
        was, prev = prev, step                                        # _start
        fresh = (not warm) or carried is None or was is None or step <= was or K > carried
        out.append((K, 1, int(fresh), draw))
        draw += 1
        carried = K
    return out, draw


def _cases():
    for H in (1, 4, 12, 20):
        for auto_reset in (1, 0):
            for start in range(EP):
                left = EP - start
                K0 = min(H, left - 1 if auto_reset else left)
                resumes = [0] + sorted({r for r in (K0 - 1, K0, K0 + 1, 1, H) if 1 <= r <= H})
                for n_steps in range(1, left + 1):
                    for warm in (1, 0):
                        for r in resumes:
                            if r and start == 0:
                                continue      # (nothing decided before the episode's first step)
                            yield (H, warm, auto_reset, r, left, n_steps)


def _check(exe, cases):
    text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    seen = set()
    for c, line in zip(cases, out):
        steps, tail = line.split("|")
        v = [int(x) for x in steps.split()]
        got = [tuple(v[i:i + 4]) for i in range(0, len(v), 4)]
        want, planned = _agent(*c)
        assert got == want, (c, got, want)
        assert [int(x) for x in tail.split()] == [planned, planned], (c, tail)
        seen |= {(d[1], d[2]) for d in got}
    return seen


def test_schedule_header_against_the_agent_restated(tmp_path):
    cases = list(_cases())
    seen = _check(_build(tmp_path, "sched", []), cases)
    assert seen == {(0, 0), (1, 0), (1, 1)}      # idle, shifted and fresh decisions all occur
    # the shrinking horizon at the episode's end, written out: 7 steps left, H = 4, auto-reset
    want, planned = _agent(4, 1, 1, 0, 7, 7)
    assert [d[0] for d in want] == [4, 4, 4, 3, 2, 1, 0] and planned == 6


def test_schedule_header_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    try:
        exe = _build(tmp_path, "sched_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("g++ could not build the driver with -fsanitize=address,undefined")
    _check(exe, list(_cases()))
