"""Tests-only restatement of `CarbonLoadEnv.step` (envs/carbon_ls.py:172-324) with the reference's own data structure: a deque of
task timestamps, popped from the left (TEST INFRASTRUCTURE, never imported by the product).  The product keeps prefix counts in a
per-env table and SEARCHES for the oldest task (csrc/sdc_physics.hpp ls_algebra / ls_ages, csrc/sdc_pairstep.hpp, csrc/sdc_wide.hip);
this model has no table, no prefix count and no search, so it can hold that search to account.

Two liberties, neither of which changes a value:
  * a timestamp is the step of the episode, not (day, hour): the reference's age `(day - task.day) * 24 + (hour - task.hour)` (:208,
    :282) is 0.25 * (t - task_step) exactly, the hour moving in quarters (sustaindc_env.py:533-621 sets the date before the step);
  * the tasks of one step carry the same timestamp (`extend([task] * n)`, :239), so the deque holds [step, count] runs.  The overdue
    `remove()` loop (:225-226) removes the first task equal to each overdue task: the oldest ones, the deque being in time order.

`run_env` also returns the case flags of tests/queue_cases.py: which rare path each env-step took, from the deque alone."""
from collections import deque

import math

import numpy as np

INT_COLS = ("tasks_in_queue", "tasks_dropped", "tasks_processed", "overdue_penalty", "computed_tasks")
FLAGS = ("overdue", "od_limited", "od_popped_no_process", "dropped", "full", "far32", "far16", "last_bin", "refill", "drain_blocked")
AGE_BINS = (24, 48, 72, 96)      # [0, 6, 12, 18, 24, inf] hours (:64) in steps; np.histogram closes the last bin: 24 h is in it


def run_env(workload, a_ls, queue_max_len):
    """One episode of one env: workload [T] (fp64, the step's `self.workload`), a_ls [T] in {0, 1, 2}.
    -> dict of per-step arrays: INT_COLS (int64), oldest / average (`ls_oldest_task_age`, `ls_average_task_age`: already / 24, fp64),
    hist [T, 5], util (`ls_shifted_workload`), head (step of the oldest queued task, -1: queue empty), overdue_processed (the
    overdue tasks the step served, :224), enqueued (the tasks it queued, :235), moved (by how many steps the oldest task
    moved, the queue non-empty before and after the step; else 0), and FLAGS (bool)."""
    T = len(a_ls)
    out = {k: np.zeros(T, np.int64) for k in INT_COLS}
    out.update(oldest=np.zeros(T), average=np.zeros(T), hist=np.zeros((T, 5)), util=np.zeros(T), head=np.full(T, -1, np.int64),
               overdue_processed=np.zeros(T, np.int64), enqueued=np.zeros(T, np.int64),
               moved=np.zeros(T, np.int64))
    out.update({k: np.zeros(T, bool) for k in FLAGS})
    q = deque()            # [step, count] runs, oldest first
    qlen = 0
    was_emptied = False    # the queue held tasks earlier in this episode and ran empty since
    for t in range(T):
        wl, a = float(workload[t]), int(a_ls[t])
        head0 = q[0][0] if q else -1
        ns = int(math.ceil(wl * (1 - 0.2) * 100))          # :194 (flexible_workload_ratio 0.2: the class default)
        shf = int(math.floor(wl * 0.2 * 100))              # :195
        dropped = processed = add = 0
        overdue = sum(n for s, n in q if (t - s) * 0.25 > 24)        # :208-209
        avail = 90 - (ns + shf)                            # :212
        od_proc = 0
        if avail > 0 and overdue > 0:                      # :217-226
            od_proc = min(overdue, avail)
            qlen -= _pop_left(q, od_proc)
        avail = 90 - (ns + shf + od_proc)                  # :229
        if a == 0:                                         # :231-242
            add = min(shf, queue_max_len - qlen)
            dropped = shf - add
            if add > 0:
                q.append([t, add])
                qlen += add
            util = (od_proc + (shf - add)) / 100
        elif a == 2:                                       # :244-264
            if avail >= 1:
                processed = min(shf, avail, qlen)
                qlen -= _pop_left(q, processed)
                util = (shf + processed + od_proc) / 100
            else:
                util = (shf + od_proc) / 100
        else:                                              # :266-268
            util = (shf + od_proc) / 100
        util += ns / 100                                   # :275-276
        hist = np.zeros(5)
        oldest = average = 0.0
        if qlen > 0:                                       # :281-284
            ages = [((t - s) * 0.25, n) for s, n in q]
            oldest = max(x for x, _ in ages)
            average = sum(x * n for x, n in ages) / qlen   # (multiples of 0.25 h: the sum is exact in any order)
            for s, n in q:                                 # :63-73
                hist[sum((t - s) >= b for b in AGE_BINS)] += n
        hist = hist / max(qlen, 1)
        hist[4] = 1 if hist[4] > 0 else 0
        out["tasks_in_queue"][t], out["tasks_dropped"][t], out["tasks_processed"][t] = qlen, dropped, processed
        out["overdue_penalty"][t], out["computed_tasks"][t] = overdue, int(util * 100)      # :306-307
        out["oldest"][t], out["average"][t], out["hist"][t], out["util"][t] = oldest / 24, average / 24, hist, util    # :304-305
        head1 = q[0][0] if q else -1
        out["head"][t], out["overdue_processed"][t], out["enqueued"][t] = head1, od_proc, add
        moved = head1 - head0 if head0 >= 0 and head1 >= 0 else 0
        out["moved"][t] = moved
        out["overdue"][t] = overdue > 0
        out["od_limited"][t] = od_proc < overdue
        out["od_popped_no_process"][t] = od_proc > 0 and a != 2
        out["dropped"][t] = a == 0 and dropped > 0
        out["full"][t] = qlen == queue_max_len
        out["far32"][t] = a == 2 and moved > 32
        out["far16"][t] = a == 2 and moved > 16
        out["last_bin"][t] = hist[4] > 0
        out["refill"][t] = was_emptied and head0 < 0 and head1 >= 0
        out["drain_blocked"][t] = a == 2 and avail < 1
        if head0 >= 0 and head1 < 0:
            was_emptied = True
    return out


def _pop_left(q, k):
    """popleft() k times (:257-258; `clear()` when that is everything, :253-254); -> k"""
    left = k
    while left > 0:
        if q[0][1] <= left:
            left -= q.popleft()[1]
        else:
            q[0][1] -= left
            left = 0
    return k


def run_batch(W, cursors, a_ls, queue_max_len):
    """Every env of a batch over one episode: W the year's workload table (fp64), cursors [N] each env's first table index,
    a_ls [T, N].  -> the dict of `run_env` with a leading [T, N] on every array."""
    T, N = a_ls.shape
    per_env = [run_env(W[int(c):int(c) + T], a_ls[:, i], queue_max_len) for i, c in enumerate(cursors)]
    return {k: np.stack([r[k] for r in per_env], axis=1) for k in per_env[0]}


def far_moves(head, a_ls=None, more_than=32):
    """Steps at which the oldest task moved by more than `more_than` steps, the queue non-empty before and after (head: `run_env`'s,
    any leading shape [T, ...]); a_ls given: under "process" only."""
    h0, h1 = head[:-1], head[1:]
    m = (h0 >= 0) & (h1 >= 0) & (h1 - h0 > more_than)
    return m if a_ls is None else m & (np.asarray(a_ls)[1:] == 2)
