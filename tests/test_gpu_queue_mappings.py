"""The load-shifting queue's rare paths on EVERY step mapping (envs/carbon_ls.py:172-324).  The device keeps prefix counts in a per-env
table and searches it for the oldest task -- a search written three times (csrc/sdc_pairstep.hpp: 32 prefetched entries and a 32-ary
search on the two-env / general mapping, two entries per lane, a parity-selected ds_bpermute and a 16-ary search on the four-env one;
csrc/sdc_wide.hip: 16 entries in registers and a table walk on the lane-per-env kernel) and run in a further launch shape by the
multi-step kernels of csrc/sdc_rollout.hip.  The scripted actions of tests/queue_cases.py take 256 envs through overdue tasks (served
in full, limited by the free capacity, popped under "defer" and "idle"), a full queue and dropped tasks, an oldest task that moves
past the prefetched entries with the queue still non-empty, the last age bin, queues that run empty and refill, "process" without
capacity -- over a 288-step episode and 120 steps of the next, so that anything an episode boundary leaves behind shows too.

Every env, every step is held to tests/queue_model.py (a deque; tests/test_queue_model.py holds it to the reference's recorded
episodes and to the oracle): the integer columns exactly, the oldest and the average age at the fp32 value of the model's fp64
result, the histogram within 1e-7, no fault; two envs of every pattern are held to the fp64 oracle at 1e-5 on obs / rew / info
(tests/production_rig.py).  The final queue table and the queue fields of the record are held to the model and, with the info block's
queue columns of every step, to the general mapping's bit for bit.  The conditions on the inputs (queue_cases.assert_conditions; the
counts stand in tests/test_queue_model.py) are asserted again here, after the device's own cursors were held to the draws the model
ran on.  Out of reach: a second round of the 32-ary / 16-ary search (queue_cases.py).

Measured on an MI355X: the file's 13 cases take 27 s together (the general mapping's first case 5.4 s, the model's 2.5 s on the CPU
included; every other 408-step case 2.1-3.2 s, every 150-step case about 0.9 s); the worst histogram error is 3.0e-8, the worst
utilisation error 5.4e-8, the oracle's bars are met at 2.8e-7."""
import functools

import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import gpu_helpers as G
from tests import queue_cases as QC
from tests import queue_model as QM
from tests.production_rig import ProductionRig
from tests.step_paths import GENERAL, KERNEL_NAME, PAIR, QUAD, WIDE

pytestmark = pytest.mark.gpu

MAPPINGS = ("general", "pair", "quad", "wide", "wide_gen")
FLAGS = {"general": GENERAL, "pair": PAIR, "quad": QUAD, "wide": WIDE, "wide_gen": WIDE}
# the lane-per-env kernel's general form serves batches of several configs (tests/step_paths.py expected_mapping)
FILES = {"wide_gen": ("dc_config.json", "dc_config_r25.json")}
# (sample geometry, debug_flags) -> the multi-step kernel (tests/step_paths.py ROLLOUT_CASES at 256 envs)
ROLLOUTS = {"sdc_rollout_fast_kernel": ("pair", 0), "sdc_rollout_quad_kernel": ("quad", QUAD), "sdc_rollout_kernel": ("general", GENERAL)}
CHUNK = 24
LS_COLS = 16                          # info[:, :16]: the load-shifting block (dc_rl_amd/_lib.py INFO_COLS)
R_Q = slice(4, 10)                    # csrc/sdc_device.hpp SdcRec: R_QPOPPED, R_QCUM, R_QCUMT, R_QHEAD, R_QCUM_HM1, R_QCUMT_HM1
UTIL_TOL = 2e-6                       # tests/test_gpu_golden.py: an fp32 info column against its fp64 reference
I = L.INFO_IDX


def make_rig(mapping, flags, queue_max_len):
    return ProductionRig(QC.N, mapping, debug_flags=flags, episode_steps=QC.EPISODE, seed=QC.SEED, n_random=0,
                         sample=QC.oracle_sample(), dc_files=FILES.get(mapping), day_range=(QC.DAY_LO, QC.DAY_HI),
                         queue_max_len=None if queue_max_len == 1000 else queue_max_len)


def check_cursors(rig, want):
    """the model ran on the windows the device draws: every env's cursor, right after its reset"""
    np.testing.assert_array_equal(rig.eng.get_state("cursor"), want)


def hold_to_model(ls, m, what):
    """ls [T, N, 16] (fp32, the info block's load-shifting columns of every env and step) against the model's arrays [T, N]"""
    T = ls.shape[0]
    for k in QM.INT_COLS:
        got, want = ls[:, :, I["ls_" + k]], m[k][:T].astype(np.float32)
        bad = np.argwhere(got != want)
        assert not len(bad), (what, k, len(bad), "first at (step, env)", bad[0].tolist(), "pattern", QC.pattern_of(int(bad[0][1])),
                              float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
    for k, col in (("oldest", "ls_oldest_task_age"), ("average", "ls_average_task_age")):
        # fp64 on the device as in the model, correctly rounded divisions of the same integers: the same double, the same float
        got, want = ls[:, :, I[col]], m[k][:T].astype(np.float32)
        bad = np.argwhere(got != want)
        assert not len(bad), (what, col, len(bad), "first at (step, env)", bad[0].tolist(), "pattern", QC.pattern_of(int(bad[0][1])),
                              float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
    h0 = I["ls_task_age_hist0"]
    eh = np.abs(ls[:, :, h0:h0 + 5].astype(np.float64) - m["hist"][:T])
    assert eh.max() <= 1e-7, (what, "histogram", np.unravel_index(eh.argmax(), eh.shape), float(eh.max()))
    eu = G.rel_err(ls[:, :, I["ls_shifted_workload"]], m["util"][:T])
    assert eu.max() <= UTIL_TOL, (what, "utilisation", np.unravel_index(eu.argmax(), eu.shape), float(eu.max()))
    return dict(hist=float(eh.max()), util=float(eu.max()))


def hold_state_to_model(qtab, rec, m, steps, what):
    """The queue table and the record's queue fields after `steps` steps: entry t of the table is (tasks ever queued up to step t of
    the episode, the sum of their steps) -- steps the second episode has not reached yet still hold the first episode's."""
    ep2 = steps > QC.EPISODE
    n2 = steps - QC.EPISODE if ep2 else 0
    n1 = min(steps, QC.EPISODE)
    add = m["enqueued"]
    t1 = np.arange(n1, dtype=np.uint64)[:, None]
    cum = np.cumsum(add[:n1], axis=0)
    cumT = np.cumsum(add[:n1].astype(np.uint64) * t1, axis=0)
    if ep2:
        t2 = np.arange(n2, dtype=np.uint64)[:, None]
        c2, cT2 = np.cumsum(add[QC.EPISODE:steps], axis=0), np.cumsum(add[QC.EPISODE:steps].astype(np.uint64) * t2, axis=0)
        cum, cumT = np.concatenate([c2, cum[n2:]]), np.concatenate([cT2, cumT[n2:]])
    np.testing.assert_array_equal(qtab[:, :n1, 0], cum.T.astype(np.uint32), err_msg=f"{what}: queue table, counts")
    np.testing.assert_array_equal(qtab[:, :n1, 1], (cumT.T & np.uint64(0xFFFFFFFF)).astype(np.uint32), err_msg=f"{what}: queue table, step sums")
    now = (n2 if ep2 else n1) - 1                 # the episode step of the last step taken
    q = rec[:, R_Q].astype(np.int64)
    qlen, head = m["tasks_in_queue"][steps - 1], m["head"][steps - 1]
    np.testing.assert_array_equal(q[:, 1], cum[now], err_msg=f"{what}: R_QCUM")
    np.testing.assert_array_equal(q[:, 0], cum[now] - qlen, err_msg=f"{what}: R_QPOPPED")
    np.testing.assert_array_equal(q[:, 2], (cumT[now] & np.uint64(0xFFFFFFFF)).astype(np.int64), err_msg=f"{what}: R_QCUMT")
    np.testing.assert_array_equal(q[:, 3], np.where(qlen > 0, head, now), err_msg=f"{what}: R_QHEAD")
    full = qlen > 0
    e = np.arange(QC.N)
    before = np.maximum(head - 1, 0)
    np.testing.assert_array_equal(q[full, 4], np.where(head > 0, cum[before, e], 0)[full], err_msg=f"{what}: R_QCUM_HM1")
    want_T = np.where(head > 0, cumT[before, e] & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    np.testing.assert_array_equal(q[full, 5], want_T[full], err_msg=f"{what}: R_QCUMT_HM1")


def finish(rig, ls, queue_max_len, steps, what):
    """The checks every run ends with; -> the host copy the mappings are compared on."""
    m, _, _ = QC.model_case(QC.SEED, queue_max_len, steps)
    worst = hold_to_model(ls, m, what)
    qtab, rec = rig.eng.get_state("qtab"), rig.eng.get_state("record")
    hold_state_to_model(qtab, rec, m, steps, what)
    rig.assert_ok()
    assert rig.resets == (1 if steps > QC.EPISODE else 0)
    print(f"{what}: {rig.eng.last_step_kernel()}, {steps} steps x {QC.N} envs on the model (worst {worst}), {len(rig.orcs)} on the oracle "
          f"(worst {rig.worst})")
    kept = dict(ls=ls, qtab=qtab[:, :min(steps, QC.EPISODE)].copy(), rec=rec[:, R_Q].copy())
    rig.eng.close()
    return kept


def assert_inputs_reach_the_cases(queue_max_len, steps):
    m, _, _ = QC.model_case(QC.SEED, queue_max_len, steps)
    if queue_max_len == 1000:
        QC.assert_conditions(m)
    else:
        assert QC.clamp_after_overdue(m, QC.actions()[:steps, :, 0]).sum() >= 100


def run_single_steps(mapping, queue_max_len, steps):
    import torch
    assert_inputs_reach_the_cases(queue_max_len, steps)
    _, c1, c2 = QC.model_case(QC.SEED, queue_max_len, steps)
    rig = make_rig(mapping, FLAGS[mapping], queue_max_len)
    obs, _ = rig.eng.reset()
    check_cursors(rig, c1)
    rig.begin_all(obs)
    acts = torch.from_numpy(QC.actions()[:steps].copy()).cuda()
    ls = torch.empty((steps, QC.N, LS_COLS), dtype=torch.float32, device="cuda")
    for t in range(steps):
        out = rig.step(acts[t])             # (asserts the kernel on the first step, no fault in any env on every step)
        ls[t] = out[4][:, :LS_COLS]
        if t == QC.EPISODE - 1:
            check_cursors(rig, c2)
    assert rig.kernel_checked and rig.eng.last_step_kernel() == KERNEL_NAME[mapping]
    return finish(rig, ls.cpu().numpy(), queue_max_len, steps, f"{mapping}, queue_max_len {queue_max_len}")


@functools.lru_cache(maxsize=None)
def general_copy(queue_max_len, steps):
    """The general mapping's run (with every check of its own), kept on the host for the other mappings to be compared with"""
    return run_single_steps("general", queue_max_len, steps)


def same_bits(kept, queue_max_len, steps, what):
    ref = general_copy(queue_max_len, steps)
    for k in ("ls", "qtab", "rec"):
        a, b = ref[k].view(np.uint32), kept[k].view(np.uint32)
        bad = np.argwhere(a != b)
        assert not len(bad), (what, k, "differs from the general mapping's", len(bad), "first at", bad[0].tolist())


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_queue_paths_single_steps_on_every_mapping(mapping):
    kept = general_copy(1000, QC.STEPS) if mapping == "general" else run_single_steps(mapping, 1000, QC.STEPS)
    same_bits(kept, 1000, QC.STEPS, mapping)


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_small_queue_clamps_after_overdue_pops_on_every_mapping(mapping):
    """queue_max_len 64, 150 steps: the queue is full from the first steps on, so that `min(shf, queue_max - qlen)` works on the
    length the overdue pops of the same step have just left."""
    args = (QC.SMALL_QUEUE, QC.SMALL_STEPS)
    kept = general_copy(*args) if mapping == "general" else run_single_steps(mapping, *args)
    same_bits(kept, *args, mapping)


@pytest.mark.parametrize("kernel", sorted(ROLLOUTS))
def test_queue_paths_in_the_multi_step_kernels(kernel):
    """The same actions through `rollout` in chunks of 24 steps (the twelfth ends the episode inside its last step)."""
    import torch
    mapping, flags = ROLLOUTS[kernel]
    assert_inputs_reach_the_cases(1000, QC.STEPS)
    _, c1, c2 = QC.model_case()
    rig = make_rig(mapping, flags, 1000)
    eng = rig.eng
    obs, _ = eng.reset()
    check_cursors(rig, c1)
    rig.begin_all(obs)
    acts = torch.from_numpy(QC.actions().copy()).cuda()
    ls = torch.empty((QC.STEPS, QC.N, LS_COLS), dtype=torch.float32, device="cuda")
    for t0 in range(0, QC.STEPS, CHUNK):
        seq = acts[t0:t0 + CHUNK].contiguous()
        out = eng.rollout(seq)
        assert eng.last_step_kernel() == kernel, (t0, eng.last_step_kernel())
        rig.check_rollout(seq, out)
        ls[t0:t0 + CHUNK] = out[4][:, :, :LS_COLS]
        if eng.steps_to_episode_end() == rig.steps:
            rig.resets += 1
            check_cursors(rig, c2)
            rig.begin_all(out[0][-1])
    kept = finish(rig, ls.cpu().numpy(), 1000, QC.STEPS, kernel)
    same_bits(kept, 1000, QC.STEPS, kernel)
