"""tests/queue_model.py (the deque restatement of CarbonLoadEnv.step, envs/carbon_ls.py:172-324) held to the reference's own
recorded episodes and to the fp64 oracle, and the scripted cases of tests/queue_cases.py held to the conditions that make them worth
running -- all without a GPU.

What the model counts on the device's own episode windows (256 envs, 288 + 120 steps, queue_max_len 1000, seed 4242, start days over
the whole year), against the least the cases must give (queue_cases.MIN_COUNTS):

    overdue tasks present                                   7802 env-steps   (>= 2000)
    overdue tasks exceed the free capacity                   933             (>= 200)
    overdue tasks popped under "defer" or "idle"            6939             (>= 2000)
    a deferring step drops tasks                             430             (>= 100)
    the queue exactly full after the step                    483             (>= 100)
    "process" moves the oldest task by > 32 steps             88             (>= 40)   (queue non-empty afterwards)
    "process" moves the oldest task by > 16 steps            230             (>= 40)
    last age bin non-empty (a task of 96 steps or more)     7861             (>= 2000)
    the queue ran empty earlier and refills                 1699             (>= 300)
    "process" with avail < 1                                 200             (>= 20)
    the oldest task moves by exactly 15 / 16 / 31 / 32 steps  88 / 82 / 70 / 54  (>= 20 each; queue non-empty afterwards)

and at queue_max_len 64 over 150 steps: 7093 env-steps drop tasks, 9011 end with a full queue, 172 defer into the full queue right
after overdue tasks were popped from it.  The oldest task is never older than 113 steps: a search range that needs a second round
of the device's 32-ary / 16-ary search cannot be reached (queue_cases.py)."""
import numpy as np
import pytest

from dc_rl_amd import dc_config, traces
from oracle import pyoracle as po
from tests import queue_cases as QC
from tests import queue_model as QM
from tests.conftest import GOLDEN_DIR
from tests.gpu_helpers import rel_err

# the load-shifting columns of tests/test_gpu_golden.py EXACT_INFO (a test file does not import another)
EXACT_INFO = ("ls_tasks_in_queue", "ls_tasks_dropped", "ls_tasks_processed", "ls_overdue_penalty", "ls_computed_tasks")
FIXTURES = ("ny_m0_defer", "ca_m3_defer_drain", "il_m1_process", "ny_m6_random")
MODEL_OF_KEY = {"ls_tasks_in_queue": "tasks_in_queue", "ls_tasks_dropped": "tasks_dropped", "ls_tasks_processed": "tasks_processed",
                "ls_overdue_penalty": "overdue_penalty", "ls_computed_tasks": "computed_tasks", "ls_oldest_task_age": "oldest",
                "ls_average_task_age": "average", "ls_shifted_workload": "util"}
EXPECTED_COUNTS = dict(overdue=7802, od_limited=933, od_popped_no_process=6939, dropped=430, full=483, far32=88, far16=230,
                       last_bin=7861, refill=1699, drain_blocked=200)


@pytest.mark.parametrize("name", FIXTURES)
def test_model_replays_the_references_recorded_episodes(name):
    """The fixture's workload window and recorded a_ls through the model: the integer columns of test_gpu_golden.EXACT_INFO exactly,
    the ages and the utilisation at that test's 2e-6, the histogram at its 1e-7."""
    d = np.load(f"{GOLDEN_DIR}/{name}.npz")
    keys = [str(k) for k in d["meta_info_keys"]]
    steps = int(d["meta_steps"])
    for ep in range(int(d["meta_episodes"])):
        pre = f"ep{ep}_"
        c0, lo = int(d[pre + "cursor0"]), int(d[pre + "win_lo"])
        m = QM.run_env(d[pre + "W"][c0 - lo:c0 - lo + steps], d[pre + "actions"][:, 0], int(d["static_queue_max_len"]))
        ginfo = d[pre + "info"]
        np.testing.assert_array_equal(d[pre + "W"][c0 - lo:c0 - lo + steps], ginfo[:, keys.index("ls_original_workload")])
        for key, col in MODEL_OF_KEY.items():
            ref = ginfo[:, keys.index(key)]
            if key in EXACT_INFO:
                np.testing.assert_array_equal(m[col], ref, err_msg=key)
            else:
                e = rel_err(m[col], ref)
                assert e.max() <= 2e-6, (name, ep, key, int(e.argmax()), float(e.max()))
        np.testing.assert_allclose(m["hist"], d[pre + "age_hist"], rtol=0, atol=1e-7)


@pytest.fixture(scope="module")
def ny():
    tb = traces.synthetic_tables("ny", 0)
    p = dc_config.size_datacenter("dc_config.json", 1, traces.max_ambient_for_sizing(traces.obtain_paths("ny")[0]))
    return tb, p


@pytest.mark.parametrize("queue_max_len,steps", [(1000, QC.STEPS), (QC.SMALL_QUEUE, QC.SMALL_STEPS)])
def test_model_equals_the_oracle_on_the_scripted_cases(ny, queue_max_len, steps):
    """Two envs of every pattern, both episodes, against oracle/sdc_oracle.c (a ring of (day, hour) stamps, scanned every step): the
    same fp64 operations on the same integers, so every queue column is equal, not close."""
    tb, p = ny
    m, c1, c2 = QC.model_case(QC.SEED, queue_max_len, steps)
    acts = QC.actions()
    cols = [(po.INFO_IDX["ls_" + k], k) for k in QM.INT_COLS]
    cols += [(po.INFO_IDX["ls_oldest_task_age"], "oldest"), (po.INFO_IDX["ls_average_task_age"], "average"),
             (po.INFO_IDX["ls_shifted_workload"], "util")]
    h0 = po.INFO_IDX["ls_hist0"]
    for i in QC.oracle_sample():
        o = po.OracleEnv(po.make_params(p["rack_n"], p["rack_full"], p["rack_idle"], p["rack_supply"], p["rack_return"],
                                        dict(p, queue_max_len=queue_max_len)))
        o.e.stpt = float(p["init_setpoint"])
        for ep, (c0, t0, n) in enumerate(((int(c1[i]), 0, min(steps, QC.EPISODE)), (int(c2[i]), QC.EPISODE, steps - QC.EPISODE))):
            if n <= 0:
                continue
            lo, hi = max(0, c0 - 16), c0 + QC.EPISODE + 18
            nc = (tb["C"][lo:hi] - tb["C"][lo:hi].min()) / np.ptp(tb["C"][lo:hi])
            nt = (tb["T"][lo:hi] - tb["T"][lo:hi].min()) / np.ptp(tb["T"][lo:hi])
            o.begin(tb["W"][lo:hi], tb["C"][lo:hi], nc, tb["T"][lo:hi], tb["WB"][lo:hi], nt, lo, c0 // 96, (c0 % 96) // 4, QC.EPISODE)
            for t in range(t0, t0 + n):
                _, _, done, info = o.step(acts[t, i])
                assert done == (t == QC.EPISODE - 1) and info[po.INFO_IDX["fault"]] == 0
                for j, k in cols:
                    assert info[j] == m[k][t, i], (QC.pattern_of(i), i, t, k, info[j], m[k][t, i])
                np.testing.assert_array_equal(info[h0:h0 + 5], m["hist"][t, i])


def test_scripted_cases_reach_every_rare_path():
    """The conditions on the inputs, from the model's own flags, on the windows the device draws (tests/reset_ref.py): the counts
    of this file's docstring, each above its bar, the overdue branch and the far move of the oldest task on every row position of a
    four-env wavefront and in every quarter of every lane-per-env wavefront."""
    m, c1, c2 = QC.model_case()
    counts = QC.assert_conditions(m)
    print("scripted cases:", counts, "oldest task at most", int(round(m["oldest"].max() * 96)), "steps old")
    assert counts == EXPECTED_COUNTS          # (the docstring's figures: a change of pattern, seed or draw scheme shows here)
    assert QC.exact_move_counts(m) == {15: 88, 16: 82, 31: 70, 32: 54}
    assert m["tasks_in_queue"].max() == 1000 and m["oldest"].max() * 96 < 128
    a_ls = QC.actions()[:, :, 0]
    for p in range(QC.SCRIPTED, 16):          # the i.i.d. patterns use all three actions
        e = [i for i in range(QC.N) if QC.pattern_of(i) == p]
        assert set(np.unique(a_ls[:, e])) == {0, 1, 2}
    # two patterns in every two-env wavefront, four in every four-env one, sixteen in every 16 lanes
    pat = np.array([QC.pattern_of(i) for i in range(QC.N)])
    assert all(len(set(pat[i:i + 2])) == 2 for i in range(0, QC.N, 2))
    assert all(len(set(pat[i:i + 4])) == 4 for i in range(0, QC.N, 4))
    assert all(len(set(pat[i:i + 16])) == 16 for i in range(0, QC.N, 16))
    # the second episode starts from an empty queue whatever the first one left
    assert (m["tasks_in_queue"][QC.EPISODE - 1] > 0).sum() > 64
    assert (m["overdue_penalty"][QC.EPISODE:QC.EPISODE + 97] == 0).all()


def test_small_queue_case_clamps_after_overdue_pops():
    m, _, _ = QC.model_case(QC.SEED, QC.SMALL_QUEUE, QC.SMALL_STEPS)
    a_ls = QC.actions()[:QC.SMALL_STEPS, :, 0]
    n = int(QC.clamp_after_overdue(m, a_ls).sum())
    c = QC.flag_counts(m)
    print("queue_max_len 64:", c, "defer into a full queue right after overdue pops:", n)
    assert (n, c["dropped"], c["full"]) == (172, 7093, 9011)
    assert m["tasks_in_queue"].max() == QC.SMALL_QUEUE
