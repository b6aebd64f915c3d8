"""The inputs of the function-level reward tests and what the sorted-list model (tests/reward_model.py) expects of each: the same
generators feed tests/test_reward_probe.py (CPU: the censuses, the model's own checks) and tests/test_gpu_reward_functions.py (the
device).  Deterministic seeds; everything is built once per process and must be left unchanged by its users.

Every generator asserts the ranges tests/aux/reward_probe.hip requires of its inputs (no case may be able to fault).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import reward_model as M

KEY_NONE, WIN, HIST = M.KEY_NONE, M.WIN, M.HIST
UP, DOWN = 1, 2
U32 = np.uint32


def _keys_of(values):
    return M.key_of(np.atleast_1d(np.asarray(values, dtype=np.float32)))


# =====================================================================================================================================
# window ops: 192 slots x 300 ops
# =====================================================================================================================================
N_SLOTS, N_OPS = 192, 300
CAPACITIES = (33, 64, 65, 100, 257)
KINDS = ("uniform", "quantised", "runs", "ramp_up", "ramp_down", "zero", "edges")
N_CORNER = 60            # slots whose first op is the full-and-ends shift's p == 0, r0 == 0 corner
N_OFF = 12               # slots with `on` false
N_BAD = 8                # slots that meet inconsistent case (a) half way
N_EMPTY = 2              # slots that start from an empty history (no window can exist: hi == 0 throughout)


def _stream(kind, rng, count):
    """float32 values of one kind."""
    if kind == "uniform":
        v = rng.normal(0.0, 50.0, count)
    elif kind == "quantised":                # few distinct keys
        v = rng.integers(0, 7, count) * 0.5 - 1.0
    elif kind == "runs":                     # long constant runs
        v = np.repeat(rng.normal(0.0, 3.0, count // 20 + 1), rng.integers(5, 60, count // 20 + 1))[:count]
        if len(v) < count:
            v = np.concatenate([v, np.full(count - len(v), v[-1])])
    elif kind == "ramp_up":
        v = np.arange(count) * 0.25 - 10.0
    elif kind == "ramp_down":
        v = 10.0 - np.arange(count) * 0.25
    elif kind == "zero":                     # values straddling zero, +-0.0 and the smallest magnitudes included
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 1.0, -1.0, 0.5, -0.5], dtype=np.float32)
        v = pool[rng.integers(0, len(pool), count)]
    else:
        v = rng.normal(0.0, 50.0, count)     # "edges": replaced op by op with keys at the window's edges
    return np.asarray(v, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def window_ops():
    """Inputs of window_ops<Form> and the model's expectation after every op.  Returns a dict of arrays (see the end)."""
    rng = np.random.default_rng(20240611)
    S, T = N_SLOTS, N_OPS
    keys0 = np.full((S, WIN), KEY_NONE, dtype=U32)
    meta = np.zeros((S, 4), dtype=np.int32)
    ops = np.zeros((S, T, 4), dtype=U32)
    iv = np.zeros((S, T, 4), dtype=U32)
    exp_keys = np.full((S, T, WIN), KEY_NONE, dtype=U32)
    exp_i = np.zeros((S, T, 12), dtype=np.int64)         # r0, hi, ch, n, ok1, a1, b1, ok3, a3, b3, span0, span1
    dead = np.zeros((S, T), dtype=bool)                  # after inconsistent case (a): only hi == 0 is expected
    bad_at = np.full(S, -1, dtype=np.int64)
    census = {o: 0 for o in M.OUTCOMES}
    census["inconsistent"] = 0
    spans_true = 0
    for s in range(S):
        corner = s < N_CORNER
        off = N_CORNER <= s < N_CORNER + N_OFF
        bad = N_CORNER + N_OFF <= s < N_CORNER + N_OFF + N_BAD
        empty = N_CORNER + N_OFF + N_BAD <= s < N_CORNER + N_OFF + N_BAD + N_EMPTY
        kind = KINDS[s % len(KINDS)]
        cap = CAPACITIES[(s // len(KINDS)) % len(CAPACITIES)]
        if corner:
            n0, cap = 64, (257, 100, 65)[s % 3]
        elif empty:
            n0 = 0
        else:
            n0 = min(cap, (1, 2, 5, 31, 33, 63, 64, 65, 70, 100, 257)[rng.integers(0, 11)])
        vals = _stream(kind, rng, n0 + T + 1)
        fifo = list(int(k) for k in _keys_of(vals[:n0]))          # the ring's content, oldest first
        hi0 = min(n0, WIN)
        place = ("start", "end", "mid")[s % 3]
        r0 = 0 if (place == "start" or corner) else (n0 - hi0 if place == "end" else int(rng.integers(0, n0 - hi0 + 1)))
        if hi0 and not corner and rng.integers(0, 4) == 0:        # a window that lists fewer than it could
            hi0 = int(rng.integers(1, hi0 + 1))
            r0 = min(r0, n0 - hi0)
        w = M.Window(fifo, r0, hi0)
        keys0[s] = w.keys()
        meta[s] = (r0, hi0, n0, 0 if off else 1)
        bad_t = int(rng.integers(100, 200)) if bad else -1
        n = n0
        was_dead = False
        for t in range(T):
            has_old = n >= cap
            x_old = fifo[0] if has_old else 0
            x_new = int(_keys_of(vals[n0 + t:n0 + t + 1])[0])
            if corner and t == 0:
                x_new = int(_keys_of(np.float32(-1e30))[0])        # below all 64 keys of a full window that starts and ends the history
            elif kind == "edges" and w.hi > 0:
                first, last = w.hist[w.r0], w.hist[w.r0 + w.hi - 1]
                x_new = int((first, last, max(first - 1, 1), min(last + 1, KEY_NONE - 1), first, last)[rng.integers(0, 6)])
            if t == bad_t and w.hi >= 2 and not was_dead:
                # inconsistent case (a): evict a key inside the window's span that the history does not hold
                ws = w.hist[w.r0:w.r0 + w.hi]
                gaps = [a + 1 for a, b in zip(ws[:-1], ws[1:]) if b - a >= 2]
                if gaps:
                    has_old, x_old = True, gaps[len(gaps) // 2]
                    bad_at[s] = t
            ops[s, t] = (x_new, x_old, 1 if has_old else 0, 0)
            outs, ch = w.update(x_new, x_old, has_old)
            if has_old:
                if bad_at[s] != t:
                    fifo.pop(0)
                fifo.append(x_new)
            else:
                fifo.append(x_new)
                n += 1
            if "inconsistent" in outs:
                was_dead = True
            for o in outs:
                census[o] += 1
            # two intervals around the window's keys (or anywhere when there is no window)
            if w.hi > 0:
                ws = w.hist[w.r0:w.r0 + w.hi]
                pts = sorted(min(max(int(ws[int(rng.integers(0, len(ws)))]) + int(rng.integers(-1, 2)), 0), KEY_NONE - 1) for _ in range(4))
                if rng.integers(0, 8) == 0:
                    pts[0] = max(int(ws[0]) - int(rng.integers(0, 1000)), 0)
                if rng.integers(0, 8) == 0:
                    pts[3] = min(int(ws[-1]) + int(rng.integers(0, 1000)), KEY_NONE - 1)
                pts = sorted(pts)
                iv[s, t] = (pts[0], pts[2], pts[1], pts[3])
            else:
                iv[s, t] = (5, 9, 7, 11)
            exp_keys[s, t] = w.keys()
            dead[s, t] = was_dead
            if was_dead:
                exp_i[s, t, :4] = (0, 0, 0, n)
                continue
            assert len(w.hist) == n == len(fifo)
            k1, k3 = M.quartile_ranks(n)
            ok1, a1, b1 = w.resolve(k1)
            ok3, a3, b3 = w.resolve(k3)
            sp = [w.spans(int(iv[s, t, 0]), int(iv[s, t, 1])), w.spans(int(iv[s, t, 2]), int(iv[s, t, 3]))]
            for j in range(2):                     # what spans() promises, checked on the history itself
                if sp[j]:
                    assert w.lists_all_in(int(iv[s, t, 2 * j]), int(iv[s, t, 2 * j + 1]))
                    spans_true += 1
            exp_i[s, t] = (w.r0, w.hi, ch, n, ok1, a1, b1, ok3, a3, b3, sp[0], sp[1])
        assert was_dead or sorted(fifo) == w.hist
    # the crossing sums, vectorised: interval 0 with flip 0, interval 1 with flip KEY_NONE
    cross = []
    for j, flip in ((0, 0), (1, KEY_NONE)):
        lo, hi = (iv[:, :, 2 * j, None], iv[:, :, 2 * j + 1, None]) if j == 0 else (iv[:, :, 2, None], iv[:, :, 3, None])
        inside = (exp_keys >= lo) & (exp_keys < hi)
        v = np.where(inside, M.key_f64(exp_keys ^ U32(flip)), 0.0)
        c = inside.sum(axis=2)
        s1, s2 = np.zeros((S, T)), np.zeros((S, T))
        for si, ti in np.argwhere(c > 0):
            s1[si, ti] = M.exact_sum(v[si, ti])
            s2[si, ti] = M.exact_sum(v[si, ti] ** 2)      # (the square of an fp32 value is exact in fp64)
        cross.append(dict(c=c, s1=s1, s2=s2, a1=np.abs(v).sum(axis=2), a2=(v * v).sum(axis=2)))
    assert (meta[:, 1] >= 0).all() and (meta[:, 1] <= WIN).all() and (iv < KEY_NONE).all()
    on = meta[:, 3] != 0
    return dict(keys0=keys0, meta=meta, ops=ops, iv=iv, exp_keys=exp_keys, exp_i=exp_i, dead=dead, bad_at=bad_at, cross=cross,
                census=census, spans_true=spans_true, on=on, crossings=int((cross[0]["c"] > 0).sum() + (cross[1]["c"] > 0).sum()))


EXP_COLS = dict(r0=0, hi=1, ch=2, n=3, ok1=4, a1=5, b1=6, ok3=7, a3=8, b3=9, span0=10, span1=11)


def check_window_ops(form, got_keys, got_i, got_d, W=None, has_on=True, has_spans=True):
    """Hold one form's output (reward_probe.window_ops) to the model's expectation.  Raises AssertionError with the first difference;
    returns the figures the test prints.  has_on False (QTrack, which has no such flag): the slots with `on` false are held to the model like the others."""
    from tests.reward_probe import NOT_APPLICABLE, OI
    W = W or window_ops()
    E, EK = W["exp_i"], W["exp_keys"]
    S, T = E.shape[:2]
    slots = np.arange(S)
    on = W["on"] if has_on else np.ones(S, dtype=bool)
    if has_on:            # a slot with `on` false comes back untouched bit for bit: r0, hi, n and the keys it started with, changed false
        E, EK = E.copy(), EK.copy()
        off = ~on
        E[off] = 0
        E[off, :, 0], E[off, :, 1], E[off, :, 3] = W["meta"][off, 0, None], W["meta"][off, 1, None], W["meta"][off, 2, None]
        EK[off] = W["keys0"][off, None, :]
    gi = got_i.astype(np.int64)

    def col(name):
        return gi[:, :, OI[name]].astype(np.int32).astype(np.int64) if name in ("r0", "hi", "n") else gi[:, :, OI[name]]

    def first_bad(mask, what, got, want):
        mask = mask & np.isin(np.arange(S), slots)[:, None]
        if mask.any():
            s, t = (int(x) for x in np.argwhere(mask)[0])
            raise AssertionError(f"{form} slot {s} op {t}: {what}: got {got[s, t]!r}, the model has {want[s, t]!r} "
                                 f"({int(mask.sum())} slot-ops differ; op = {W['ops'][s, t].tolist()}, before: r0 hi ch n = "
                                 f"{(E[s, t - 1, :4] if t else W['meta'][s]).tolist()})")

    live = ~W["dead"]
    first_bad(col("hi") != E[:, :, 1], "hi (a window dropped or kept that the model keeps or drops)", col("hi"), E[:, :, 1])
    first_bad(live & (col("r0") != E[:, :, 0]), "r0", col("r0"), E[:, :, 0])
    first_bad(live & (col("n") != E[:, :, 3]), "n", col("n"), E[:, :, 3])
    kd = (got_keys != EK).any(axis=2)
    first_bad(live & kd, "window keys (the contract: keys[i] == sorted[r0 + i], KEY_NONE beyond hi)", got_keys, EK)
    first_bad(live & (col("ch") != E[:, :, 2]), "changed", col("ch"), E[:, :, 2])
    # changed is never false when a key register changed
    before = np.concatenate([np.broadcast_to(W["keys0"][:, None, :], (S, 1, WIN)), got_keys[:, :-1]], axis=1)
    moved = (before != got_keys).any(axis=2)
    first_bad(live & moved & (col("ch") == 0), "a key register changed and `changed` is false", col("ch"), E[:, :, 2])
    act = live & on[:, None]
    for q in ("1", "3"):
        ok = E[:, :, EXP_COLS["ok" + q]]
        first_bad(act & (col("ok" + q) != ok), "resolve ok at quartile " + q, col("ok" + q), ok)
        for nm in ("a", "b"):
            first_bad(act & (ok != 0) & (col(nm + q) != E[:, :, EXP_COLS[nm + q]]), f"resolve key {nm}{q}", col(nm + q), E[:, :, EXP_COLS[nm + q]])
    hi_pos = act & (E[:, :, 1] > 0)
    wfirst, wlast = EK[:, :, 0].astype(np.int64), np.take_along_axis(EK, np.maximum(E[:, :, 1] - 1, 0)[:, :, None], axis=2)[:, :, 0].astype(np.int64)
    first_bad(hi_pos & (col("first") != wfirst), "first key", col("first"), wfirst)
    first_bad(hi_pos & (col("last") != wlast), "last key", col("last"), wlast)
    for j in range(2):
        sp = col(f"span{j}")
        if not has_spans:                              # (the quad mapping has no spans function: its callers' first / last key above)
            assert (sp[act] == NOT_APPLICABLE).all()
            continue
        first_bad(act & (sp != E[:, :, EXP_COLS[f"span{j}"]]), f"spans of interval {j}", sp, E[:, :, EXP_COLS[f"span{j}"]])
    worst = 0.0
    for j in range(2):
        X = W["cross"][j]
        c = np.where(act, X["c"], 0)
        first_bad(act & (col(f"c{j}") != c), f"crossing count of interval {j}", col(f"c{j}"), c)
        first_bad(act & (col(f"any{j}") != (c > 0)), f"crossing flag of interval {j}", col(f"any{j}"), (c > 0).astype(np.int64))
        for k, (ref, mag) in enumerate(((X["s1"], X["a1"]), (X["s2"], X["a2"]))):
            got = got_d[:, :, 2 * j + k]
            bound = 63 * M.EPS * mag                   # (the summation bound of any 64-term tree; exact where one term crossed)
            err = np.abs(got - ref)
            first_bad(act & (c > 0) & ~(err <= bound), f"crossing sum {k + 1} of interval {j}", got, ref)
            first_bad(act & (c == 0) & (got != 0.0), f"crossing sum {k + 1} of interval {j} with nothing crossed", got, ref)
            m = act & (c > 0) & (bound > 0)
            if m.any():
                worst = max(worst, float((err[m] / bound[m]).max()))
    return dict(worst_sum_ratio=worst, over_reported=int((act & (col("ch") != 0) & ~moved).sum()))


def expected_as_output(has_on=True, spans=True):
    """The model's expectation in the probe's output layout (what a correct device returns): the checker's own test starts from it."""
    from tests.reward_probe import NOT_APPLICABLE, OI, OI_W
    W = window_ops()
    E, EK = W["exp_i"], W["exp_keys"].copy()
    S, T = E.shape[:2]
    gi = np.zeros((S, T, OI_W), dtype=np.int64)
    for name, c in EXP_COLS.items():
        gi[:, :, OI[name]] = E[:, :, c]
    if not spans:
        gi[:, :, OI["span0"]] = gi[:, :, OI["span1"]] = NOT_APPLICABLE
    gi[:, :, OI["first"]] = EK[:, :, 0]
    gi[:, :, OI["last"]] = np.take_along_axis(EK, np.maximum(E[:, :, 1] - 1, 0)[:, :, None], axis=2)[:, :, 0]
    gd = np.zeros((S, T, 4))
    for j in range(2):
        X = W["cross"][j]
        gi[:, :, OI[f"c{j}"]], gi[:, :, OI[f"any{j}"]] = X["c"], X["c"] > 0
        gd[:, :, 2 * j], gd[:, :, 2 * j + 1] = X["s1"], X["s2"]
    if has_on:
        off = ~W["on"]
        gi[off] = 0
        gi[off, :, OI["r0"]], gi[off, :, OI["hi"]], gi[off, :, OI["n"]] = W["meta"][off, 0, None], W["meta"][off, 1, None], W["meta"][off, 2, None]
        EK[off] = W["keys0"][off, None, :]
        gd[off] = 0.0
    return EK, (gi & 0xFFFFFFFF).astype(U32), gd


# =====================================================================================================================================
# rings
# =====================================================================================================================================
def make_ring(hist_keys, rng, scatter=True):
    """A ring of HIST slots holding the keys in random slots, KEY_NONE elsewhere (scattered, or all at the end)."""
    n = len(hist_keys)
    assert 2 <= n <= HIST
    ring = np.full(HIST, KEY_NONE, dtype=U32)
    slots = rng.permutation(HIST)[:n] if scatter else rng.permutation(n)
    ring[slots] = np.asarray(hist_keys, dtype=U32)[rng.permutation(n)]
    return ring


def _lane_of_slot(slot, coop):
    """The lane list a ring slot belongs to: (wavefront, lane) -- one wavefront reads dwordx4 number q * 64 + lane for q < 40; of the four
    cooperating ones wavefront v takes q in [10 v, 10 v + 10)."""
    vec = slot >> 2
    q, lane = vec // 64, vec % 64
    return (q // 10 if coop else 0) * 64 + lane


def refill_rounds(ring, win, patch_slot, patch_x, n, r0, hi, direction, side, k, coop):
    """The rounds a refill of this case takes and whether one of them meets D == 0, by the header's description of the sweep (the lanes'
    4-smallest lists; used for the CENSUS of the inputs only, never as the reference of an output)."""
    r = ring.astype(np.uint64).copy()
    if patch_slot >= 0:
        r[patch_slot] = patch_x
    fd = KEY_NONE if direction == DOWN else 0
    f = fd ^ side
    x = r ^ np.uint64(f)
    pivot = int(win[hi - 1])                      # the window's last key in the space where it grows upwards
    if fd:
        pivot = KEY_NONE - int(win[0])
        r0 = n - (r0 + hi)
        k = n - 1 - k
    n_empty = HIST - n if f else 0
    top = r0 + hi
    s = min(max(k - WIN // 2 - r0, 0), hi - 1)
    kept = hi - s
    filled = kept
    lanes = _LANES[coop]
    rounds, d0 = 0, False
    for _ in range(8):
        if not (filled < WIN and top < n):
            break
        rounds += 1
        pp = pivot + 1
        smax = KEY_NONE - pp
        d = (x - np.uint64(pp)) & np.uint64(KEY_NONE)
        cnt = int((x <= pivot).sum())
        order = np.lexsort((d, lanes))
        ds, ls = d[order], lanes[order]
        starts = np.flatnonzero(np.r_[True, ls[1:] != ls[:-1]])
        e3 = ds[starts + 3]                               # every lane list holds at least 40 keys
        D = min(int(e3.min()), smax)
        extra = cnt - n_empty - top
        if extra < 0:
            return dict(rounds=rounds, d0=d0, dropped=True)
        m = int((d < D).sum())
        d0 = d0 or D == 0
        filled += extra + m
        top += extra + m
        if D >= smax or filled - kept >= 12:
            break
        pivot = pp + D
    return dict(rounds=rounds, d0=d0, dropped=filled <= kept)


_LANES = {c: np.array([_lane_of_slot(i, c) for i in range(HIST)]) for c in (False, True)}


def ring_hist_space(ring, patch_slot, patch_x, side):
    """The history in the window's own key space (complemented for the lower clip bound's window), sorted."""
    return np.sort(M.ring_history(ring, patch_slot, patch_x) ^ U32(side))


@functools.lru_cache(maxsize=None)
def refill_cases():
    """256 rings with a window each: dict of arrays ring [256][HIST], win [256][64], meta [256][8] and per-case notes."""
    rng = np.random.default_rng(777)
    N = 256
    ring = np.empty((N, HIST), dtype=U32)
    win = np.full((N, WIN), KEY_NONE, dtype=U32)
    meta = np.zeros((N, 8), dtype=np.int64)
    notes = []
    ns = (65, 100, 1500, 10000, 10240)
    runs = (1, 4, 5, 63, 64, 300)
    # every (hi, t) for which qt_refill_ahead asks for a refill at margins (3, 6) and (10, 10), dealt round the cases
    his = (13, 14, 20, 33, 47, 63, 64)
    combos = []
    for m_lo, m_hi in ((3, 6), (10, 10)):
        for hi in his:
            for t in range(hi - m_hi + 1, hi):
                combos.append((UP, hi, t, m_lo, m_hi))
            for t in range(0, m_lo):
                if t <= hi - m_hi:                             # (beyond that the test asks for UP first)
                    combos.append((DOWN, hi, t, m_lo, m_hi))
    combos = [combos[i] for i in rng.permutation(len(combos))]
    for c in range(N):
        n = ns[c % 5]
        direction, hi, t, m_lo, m_hi = combos[c % len(combos)]
        side = KEY_NONE if (c // 5) % 2 else 0
        feature = ("plain", "few_beyond", "far_edge", "run", "d0", "all_equal", "sign", "patch_in", "patch_pivot", "patch_far",
                   "inconsistent")[c % 11] if c >= 22 else ("run", "d0")[c % 2]
        run_len = runs[(c // 11) % 6] if feature == "run" else 0
        if (feature in ("run", "d0") and n - hi < 16) or (feature.startswith("patch") and n < 1500):
            n = 1500                                           # (room beyond the window for the run / for a slot to patch)
        # the history in the WINDOW's space, growing upwards in the direction of the refill ("work space": for DOWN the complement)
        if feature == "all_equal":
            work = np.full(n, 0x80001234, dtype=np.uint64)
        elif feature == "sign":
            work = np.sort(rng.integers(0x7FFFFF00, 0x80000100, n).astype(np.uint64))      # keys crossing 0x7FFFFFFF / 0x80000000
        else:
            work = np.sort(rng.integers(0x30000000, 0xD0000000, n).astype(np.uint64))
            if c % 3 == 0:
                work = np.sort(rng.integers(0x80000000, 0x80000000 + 4 * n, n).astype(np.uint64))   # dense: ties and neighbours
        # window ranks in work space (ascending, growing upwards)
        if feature == "few_beyond":
            beyond = int(rng.integers(1, 12))
        elif feature == "far_edge":
            beyond = None
        else:
            beyond = int(rng.integers(40 if feature.startswith("patch") else 12, max(41, n - hi)))
        if feature == "far_edge":
            r0w = 0                                            # the window already touches the history's far end
        else:
            r0w = max(n - hi - beyond, 1)
        if r0w + hi >= n:
            r0w = n - hi - 1
        assert r0w >= 0 and r0w + hi < n
        top = r0w + hi
        pivot = int(work[top - 1])
        run_key = 0
        if feature == "run" or feature == "d0":
            L = 4 if feature == "d0" else run_len
            L = min(L, n - top)
            # a run of equal keys just beyond the pivot: at pivot + 1 (a lane that holds four of them makes the round's D zero), or a
            # little further with nothing in between
            run_key = pivot + 1 + (0 if feature == "d0" else (0, 1, 5)[(c // 2) % 3])
            work[top:top + L] = run_key
            work[top + L:] = np.maximum(work[top + L:], run_key + 1 + np.arange(n - top - L, dtype=np.uint64))
            work = np.sort(work)
        if feature == "inconsistent":
            work[top:] = np.maximum(work[top:], np.uint64(pivot + 1))   # (no copy of the pivot beyond the window: a missing key shows)
        # rank wanted: t counts from the window's first rank in the ORIGINAL orientation
        tw = t if direction == UP else hi - 1 - t
        kw = r0w + tw
        # back to the window's own space and to ring keys
        if direction == UP:
            own, r0 = work, r0w
        else:
            own, r0 = np.sort(np.uint64(KEY_NONE) - work), n - (r0w + hi)
        k = r0 + t
        assert (own[r0 + np.arange(hi)] == (work[r0w:r0w + hi] if direction == UP else (np.uint64(KEY_NONE) - work[r0w:r0w + hi])[::-1])).all()
        keys = (own ^ np.uint64(side)).astype(U32)             # what the ring holds
        assert (keys != KEY_NONE).all() and (own != KEY_NONE).all() and (own != 0).all()
        rg = make_ring(keys, rng, scatter=(c % 4 != 3))
        if feature == "d0" or (feature == "run" and run_len >= 4):
            # four copies of the run's key in ONE lane (one aligned dwordx4 of the ring holds them): the lane's list overflows, which
            # stops the round's complete part short of the run and forces a second round
            f_all = (KEY_NONE if direction == DOWN else 0) ^ side
            want = U32(run_key ^ f_all)
            at = np.flatnonzero(rg == want)
            assert len(at) >= 4, (c, len(at))
            vec = int(rng.integers(0, HIST // 4)) * 4
            for j in range(4):
                i, o = vec + j, int(at[j])
                if rg[i] != want:
                    rg[i], rg[o] = rg[o], rg[i]
            assert (rg[vec:vec + 4] == want).all()
        patch_slot, patch_x = -1, 0
        if feature.startswith("patch"):
            # the slot's memory holds a stale key; the history's key there is patch_x
            f_all = (KEY_NONE if direction == DOWN else 0) ^ side
            filled = np.flatnonzero(rg != KEY_NONE)
            # choose a filled slot on dword position c % 4 whose key is not in the window
            cand = [int(i) for i in filled if i % 4 == c % 4]
            wk = set(int(v) for v in work[r0w:r0w + hi])
            cand = [i for i in cand if (int(rg[i]) ^ f_all) not in wk and (int(rg[i]) ^ f_all) > pivot]
            patch_slot = cand[int(rng.integers(0, len(cand)))]
            old_w = int(rg[patch_slot]) ^ f_all
            if feature == "patch_in":
                new_w = pivot + 1 + int(rng.integers(0, 3))
            elif feature == "patch_pivot":
                new_w = pivot
            else:
                new_w = int(work[-1]) + 1000
            patch_x = int(new_w ^ f_all)
            # memory keeps a stale key that would land right behind the pivot if the patch were ignored
            rg[patch_slot] = U32((pivot + 1) ^ f_all) if feature == "patch_far" else U32(old_w ^ f_all)
            assert patch_x != KEY_NONE
        consistent = True
        if feature == "inconsistent":
            # inconsistent case (b): one key at or below the pivot is missing from the ring (f == 0 spaces, where an empty slot does
            # not count as a key below the pivot)
            direction_side_ok = ((KEY_NONE if direction == DOWN else 0) ^ side) == 0
            if not direction_side_ok:
                side = side ^ KEY_NONE
                keys = (own ^ np.uint64(side)).astype(U32)
                rg = make_ring(keys, rng)
            f_all = 0
            below = np.flatnonzero((rg != KEY_NONE) & ((rg.astype(np.uint64) ^ np.uint64(f_all)) <= pivot))
            rg[below[int(rng.integers(0, len(below)))]] = KEY_NONE
            consistent = False
        ring[c] = rg
        win[c, :hi] = own[r0:r0 + hi].astype(U32)
        meta[c] = (r0, hi, direction, k, n, patch_slot, patch_x, side)
        notes.append(dict(feature=feature, run_len=run_len, consistent=consistent, m_lo=m_lo, m_hi=m_hi, t=t))
        # the ranges the probe requires
        assert 1 <= hi <= WIN and 2 <= n <= HIST and -1 <= patch_slot < HIST and 0 <= k < n and 0 <= r0 and r0 + hi <= n
        if consistent:
            h = ring_hist_space(rg, patch_slot, patch_x, side)
            assert len(h) == n and (h[r0:r0 + hi] == win[c, :hi]).all(), (c, feature)
            assert M.refill_ahead(r0, hi, k, n, m_lo, m_hi) == direction, (c, feature, r0, hi, k, n)
    return dict(ring=ring, win=win, meta=meta, notes=notes)


@functools.lru_cache(maxsize=None)
def refill_census():
    R = refill_cases()
    out = dict(rounds2={False: 0, True: 0}, d0={False: 0, True: 0}, side={0: 0, KEY_NONE: 0}, dir={UP: 0, DOWN: 0}, reaches_end=0,
               inconsistent=0, dropped_consistent=0, features={})
    for c, note in enumerate(R["notes"]):
        r0, hi, direction, k, n, ps, px, side = (int(v) for v in R["meta"][c])
        out["features"][note["feature"]] = out["features"].get(note["feature"], 0) + 1
        if not note["consistent"]:
            out["inconsistent"] += 1
            for coop in (False, True):
                assert refill_rounds(R["ring"][c], R["win"][c], ps, px, n, r0, hi, direction, side, k, coop)["dropped"]
            continue
        out["side"][side] += 1
        out["dir"][direction] += 1
        beyond = (n - (r0 + hi)) if direction == UP else r0
        out["reaches_end"] += beyond < 12
        for coop in (False, True):
            rr = refill_rounds(R["ring"][c], R["win"][c], ps, px, n, r0, hi, direction, side, k, coop)
            out["rounds2"][coop] += rr["rounds"] >= 2
            out["d0"][coop] += rr["d0"]
            out["dropped_consistent"] += rr["dropped"]
    return out


def check_refill(case, keys, r0, hi, R=None):
    """Hold one refill output (one wavefront's window) to the sorted ring.  Returns None or a message."""
    R = R or refill_cases()
    note = R["notes"][case]
    r0_in, hi_in, direction, k, n, ps, px, side = (int(v) for v in R["meta"][case])
    keys = np.asarray(keys, dtype=U32)
    if not note["consistent"]:
        return None if hi == 0 else f"a ring the window does not describe: hi = {hi}, expected the window dropped"
    if hi <= 0:
        return "the window was dropped on a consistent case"
    h = ring_hist_space(R["ring"][case], ps, px, side)
    bad = M.contract_violation(keys, r0, hi, [int(v) for v in h])
    if bad:
        return bad
    if direction == UP:
        s = min(max(k - WIN // 2 - r0_in, 0), hi_in - 1)
        if r0 != r0_in + s:
            return f"r0 = {r0}: the kept part starts at rank {r0_in + s}"
        avail = n - (r0_in + hi_in)
    else:
        kk, r0m = n - 1 - k, n - (r0_in + hi_in)
        s = min(max(kk - WIN // 2 - r0m, 0), hi_in - 1)
        if r0 + hi != r0_in + hi_in - s:
            return f"the window ends at rank {r0 + hi}: the kept part ends at rank {r0_in + hi_in - s}"
        avail = r0_in
    kept = hi_in - s
    need = min(12, avail, WIN - kept)
    if hi - kept < need:
        return f"extended by {hi - kept} keys, at least {need} lie beyond"
    if not (r0 <= k and (k + 1 > n - 1 or k + 1 < r0 + hi)):
        return f"ranks {k}, {k + 1} are not inside [{r0}, {r0 + hi})"
    if M.refill_ahead(r0, hi, k, n, note["m_lo"], note["m_hi"]) == direction:
        return f"qt_refill_ahead still asks for the same refill: r0 {r0} hi {hi} k {k}"
    return None


# =====================================================================================================================================
# rebuild and bisect_build: 128 rings
# =====================================================================================================================================
REBUILD_NS = (2, 3, 31, 32, 33, 63, 64, 65, 128, 1500, 10240)


@functools.lru_cache(maxsize=None)
def rebuild_cases():
    rng = np.random.default_rng(4242)
    N = 128
    ring = np.empty((N, HIST), dtype=U32)
    meta = np.zeros((N, 4), dtype=np.int64)
    bmeta = np.zeros((N, 8), dtype=np.int64)
    hists, notes = [], []
    feats = ("normal", "ties_q", "wide_ties", "tail0", "tail_half", "tail9", "iqr0", "zero")
    for c in range(N):
        n = REBUILD_NS[c % len(REBUILD_NS)]
        feat = feats[(c // len(REBUILD_NS)) % len(feats)]
        if feat == "normal":
            v = rng.normal(0.0, 100.0, n)
        elif feat == "ties_q":                         # heavy ties at a quartile rank
            v = np.round(rng.normal(0.0, 2.0, n))
        elif feat == "wide_ties":                      # more than 64 copies of the key at a window's first or last rank
            v = rng.normal(0.0, 100.0, n)
            v.sort()
            k1, k3 = M.quartile_ranks(n)
            a, b = M.window_ranks(k1 if c % 2 else k3, n)
            e = a if (c // 2) % 2 else b
            v[max(0, e - 40):min(n, e + 41)] = v[e]
        elif feat == "tail0":                          # no key beyond a clip bound
            v = rng.uniform(-1.0, 1.0, n)
        elif feat in ("tail_half", "tail9"):           # 0.5 % / 9 % of the keys beyond the bounds
            v = rng.uniform(-1.0, 1.0, n)
            m = max(1, int(round(n * (0.005 if feat == "tail_half" else 0.09)))) if n >= 8 else 0
            idx = rng.permutation(n)[:m]
            v[idx] = rng.choice([-1.0, 1.0], m) * rng.uniform(10.0, 1e4, m)
        elif feat == "iqr0":
            v = np.full(n, 7.25)
            m = n // 5
            v[:m] = rng.normal(0.0, 50.0, m)
        else:                                          # values straddling zero
            v = rng.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 2.5]), n)
        keys = _keys_of(v)
        rg = make_ring(keys, rng, scatter=(c % 3 != 2))
        patch_slot, patch_x = -1, 0
        if c % 4 == 1:                                 # the step's own key, not yet visible in memory
            patch_slot = int(np.flatnonzero(rg != KEY_NONE)[int(rng.integers(0, n))])
            patch_x = int(rg[patch_slot])
            rg[patch_slot] = _keys_of(np.float32(12345.0))[0]
        ring[c] = rg
        meta[c] = (n, patch_slot, patch_x, 0)
        h = M.ring_history(rg, patch_slot, patch_x)
        assert len(h) == n
        hists.append(h)
        # bisect_build: windows round two ranks of the model's choosing (the extremes included)
        ks = ((0, n - 1), M.quartile_ranks(n), (n // 2, n - 1), (0, n // 3))[c % 4]
        (a1, b1), (a3, b3) = M.window_ranks(ks[0], n), M.window_ranks(ks[1], n)
        bmeta[c] = (n, a1, b1, a3, b3, 0, 0, 0)
        assert 0 <= a1 <= b1 < n and 0 <= a3 <= b3 < n and b1 - a1 < WIN and b3 - a3 < WIN
        notes.append(dict(feature=feat, n=n))
    return dict(ring=ring, meta=meta, bmeta=bmeta, hists=hists, notes=notes)


def smallest_key_with(values_pred, shape):
    """The smallest key k in [0x007FFFFF, 0xFF800000] (-inf .. +inf) with values_pred(value of k) true, by bisection on the key space;
    0xFF800001 where none has.  values_pred is monotone in the key (false ... false true ... true)."""
    lo = np.full(shape, 0x007FFFFF, dtype=np.int64)
    hi = np.full(shape, 0xFF800001, dtype=np.int64)
    for _ in range(33):
        mid = (lo + hi) >> 1
        p = values_pred(M.key_f64(mid.astype(U32)))
        hi = np.where(p, mid, hi)
        lo = np.where(p, lo, mid + 1)
        lo = np.minimum(lo, hi)
    return hi


def bound_keys_by_definition(lb, ub):
    """klb = the smallest key whose value is >= lb, kub = the smallest key whose value is > ub, then the header's clamps."""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    klb = smallest_key_with(lambda v: v >= lb, lb.shape)
    kub = smallest_key_with(lambda v: v > ub, ub.shape)
    klb = np.minimum(np.maximum(klb, 2), KEY_NONE - 2)
    kub = np.minimum(np.maximum(kub, klb), KEY_NONE - 2)
    return klb.astype(U32), kub.astype(U32)


@functools.lru_cache(maxsize=None)
def rebuild_expectations():
    """Per ring: windows, bounds, exact sums (as floats rounded once, with the sums of magnitudes for the bounds)."""
    R = rebuild_cases()
    out = []
    for c, h in enumerate(R["hists"]):
        n = len(h)
        hl = [int(x) for x in h]
        k1, k3 = M.quartile_ranks(n)
        (a1, b1), (a3, b3) = M.window_ranks(k1, n), M.window_ranks(k3, n)
        q1v, q3v, lb, ub, ctr = (float(x) for x in M.bounds_from_keys(n, *M.quartile_keys(hl)))
        klb, kub = (int(x) for x in bound_keys_by_definition(np.float64(lb), np.float64(ub)))
        v = M.key_f64(h)
        hi_m, lo_m = h >= kub, h < klb
        e = dict(n=n, q1=(a1, b1), q3=(a3, b3), lb=lb, ub=ub, ctr=ctr, klb=klb, kub=kub, qc=(int(hi_m.sum()), int(lo_m.sum())),
                 A1=M.exact_sum(v), A2=M.exact_sum(v * v), abs1=float(np.abs(v).sum()), abs2=float((v * v).sum()),
                 qs1=(M.exact_sum(v[hi_m]), M.exact_sum(v[lo_m])), qs2=(M.exact_sum(v[hi_m] ** 2), M.exact_sum(v[lo_m] ** 2)),
                 qabs1=(float(np.abs(v[hi_m]).sum()), float(np.abs(v[lo_m]).sum())), qabs2=(float((v[hi_m] ** 2).sum()), float((v[lo_m] ** 2).sum())))
        e["bu"] = M.window_ranks(n - e["qc"][0], n)
        e["bl"] = M.window_ranks(e["qc"][1], n)
        if n < M.SMALL_N:
            e["ref"] = M.clipped_reference(hl)
            f = np.clip(v, lb, ub) - ctr                  # wave_direct_moments sums the clipped values centred on ctr
            e["cen_abs"], e["m2c"] = float(np.abs(f).sum()), float((f * f).sum() / n)
        out.append(e)
    return out


def check_rebuild(case, keys, oi, od, X=None):
    """Hold one ring's rebuild_state output to the model.  keys [4][64], oi [16], od [12] as reward_probe.rebuild returns them.
    Returns (None or a message, the worst ratio of a sum's error to its bound)."""
    from tests.reward_probe import RB_D, RB_I
    e = (X or rebuild_expectations())[case]
    h = rebuild_cases()["hists"][case]
    n = e["n"]
    tiny = n < M.SMALL_N
    oi = np.asarray(oi).astype(np.int64)
    if int(oi[RB_I["ok"]]) != (0 if tiny else 1):
        return f"ok = {int(oi[RB_I['ok']])} on a consistent ring of {n} keys", 0.0

    def window(name, j, ranks, complemented=False):
        a, b = ranks
        r0, hi = int(oi[RB_I[name]]), int(oi[RB_I[name] + 1])
        want = h[a:b + 1]
        if complemented:      # the lower bound's window: complemented keys, reversed, ranks counted from the top
            want, a = (~want)[::-1], n - (b + 1)
        if (r0, hi) != (a, b - ranks[0] + 1 if not complemented else len(want)):
            return f"{name}: r0, hi = {r0}, {hi}; the model has {a}, {len(want)}"
        if (keys[j][:hi] != want).any() or (keys[j][hi:] != KEY_NONE).any():
            return f"{name}: the keys are not ranks {ranks} of the history"
        return None

    for name, j in (("q1", 0), ("q3", 1)):
        bad = window(name, j, e[name])
        if bad:
            return bad, 0.0
    for nm in ("lb", "ub", "ctr"):
        if not M.same_value_or_bits(od[RB_D[nm]], e[nm]):
            return f"{nm} = {od[RB_D[nm]]!r}, numpy's lerp gives {e[nm]!r}", 0.0
    if (int(oi[RB_I["klb"]]) & KEY_NONE, int(oi[RB_I["kub"]]) & KEY_NONE) != (e["klb"], e["kub"]):
        return f"klb, kub = {int(oi[RB_I['klb']]) & KEY_NONE:#x}, {int(oi[RB_I['kub']]) & KEY_NONE:#x}; by definition {e['klb']:#x}, {e['kub']:#x}", 0.0
    worst = 0.0
    if tiny:
        ref = e["ref"]
        mean, sd = float(od[RB_D["mean"]]), float(od[RB_D["sd"]])
        # wave_direct_moments (n < SMALL_N) sums f = clip(v) - ctr over the ring: each f rounds once, a sum of n terms in any order is
        # within (n - 1) eps sum |f|, the quotient and the final ctr + m0 round once each -- the moments bound's reasoning with the sums
        # formed here instead of handed in:  |mean - exact| <= (n + 1) eps sum |f| / n + eps |mean|
        bm = M.EPS * ((n + 1) * e["cen_abs"] / n + abs(ref["mean"]))
        if not abs(mean - ref["mean"]) <= bm:
            return f"mean = {mean!r}, exact {ref['mean']!r}: off by {abs(mean - ref['mean']):.3g}, bound {bm:.3g}", 0.0
        if ref["var"] > 1e-30 and e["ub"] > e["lb"]:
            # var = s2 / n - m0^2 on the centred values: every f^2 carries 3 eps, the sum (n - 1) eps, m0^2 <= m2c carries twice the
            # mean's error: at most (3 n + 6) eps m2c on var, half of that relative on the root, which is correctly rounded
            bs = (2 * n + 4) * M.EPS * e["m2c"] / ref["var"] + 1e-15
            if not abs(sd - ref["sd"]) <= bs * ref["sd"]:
                return f"sd = {sd!r}, exact {ref['sd']!r}: relative {abs(sd / ref['sd'] - 1):.3g}, bound {bs:.3g}", 0.0
            worst = abs(sd / ref["sd"] - 1) / bs
        elif sd != 0.0 and not abs(sd) <= 1e-15:
            return f"sd = {sd!r} where the clipped history is constant", 0.0
        return None, worst
    if (int(oi[RB_I["qc"]]), int(oi[RB_I["qc"] + 1])) != e["qc"]:
        return f"tail counts {int(oi[RB_I['qc']])}, {int(oi[RB_I['qc'] + 1])}; the history has {e['qc']}", 0.0
    for name, j, ranks, comp in (("bu", 2, e["bu"], False), ("bl", 3, e["bl"], True)):
        bad = window(name, j, ranks, comp)
        if bad:
            return bad, 0.0
    sums = (("A1", od[RB_D["A1"]], e["A1"], e["abs1"]), ("A2", od[RB_D["A2"]], e["A2"], e["abs2"]),
            ("qs1[0]", od[RB_D["qs1"]], e["qs1"][0], e["qabs1"][0]), ("qs1[1]", od[RB_D["qs1"] + 1], e["qs1"][1], e["qabs1"][1]),
            ("qs2[0]", od[RB_D["qs2"]], e["qs2"][0], e["qabs2"][0]), ("qs2[1]", od[RB_D["qs2"] + 1], e["qs2"][1], e["qabs2"][1]))
    for name, got, want, mag in sums:
        bound = (n - 1) * M.EPS * mag           # recursive summation in any order
        if not abs(float(got) - want) <= bound:
            return f"{name} = {float(got)!r}, exact {want!r}: off by {abs(float(got) - want):.3g}, bound {bound:.3g}", 0.0
        if bound > 0:
            worst = max(worst, abs(float(got) - want) / bound)
    return None, worst


def check_bisect(case, k4, keys, oi):
    """wave_bisection4's keys and windows_build's two windows of one ring against the sorted history."""
    R = rebuild_cases()
    h = M.ring_history(R["ring"][case])          # (bisect_build takes no patch: the ring as memory holds it)
    n, a1, b1, a3, b3 = (int(v) for v in R["bmeta"][case][:5])
    assert len(h) == n
    want4 = [int(h[r]) for r in (a1, b1, a3, b3)]
    if [int(x) for x in k4] != want4:
        return f"bisection keys {[hex(int(x)) for x in k4]}, sorted[rank] is {[hex(x) for x in want4]}"
    for j, (a, b) in enumerate(((a1, b1), (a3, b3))):
        r0, hi = int(oi[2 * j]), int(oi[2 * j + 1])
        if (r0, hi) != (a, b - a + 1):
            return f"window {j}: r0, hi = {r0}, {hi}; ranks {a} .. {b}"
        bad = M.contract_violation(keys[j], r0, hi, [int(x) for x in h])
        if bad:
            return f"window {j}: {bad}"
    return None


# =====================================================================================================================================
# bounds and moments: about 200 000 elements
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def bounds_cases():
    """n, a1, b1, a3, b3 (uint32 arrays): the quartile keys of the histories above, adversarial pairs, every n mod 4."""
    rng = np.random.default_rng(99)
    rows = []
    # the quartile keys of the window-op histories (after every op) and of the rebuild rings
    W = window_ops()
    E = W["exp_i"]
    m = (E[:, :, EXP_COLS["ok1"]] != 0) & (E[:, :, EXP_COLS["ok3"]] != 0) & ~W["dead"] & (E[:, :, 3] >= 2)
    rows.append(np.stack([E[:, :, 3][m], E[:, :, 5][m], E[:, :, 6][m], E[:, :, 8][m], E[:, :, 9][m]]))
    hs = rebuild_cases()["hists"]
    rows.append(np.array([[len(h), *M.quartile_keys([int(x) for x in h])] for h in hs], dtype=np.int64).T)
    # adversarial pairs: adjacent keys, equal keys, a huge gap -- with every residue of n mod 4
    N = 150_000
    n = rng.integers(2, HIST + 1, N)
    n[:4000] = 2 + (np.arange(4000) % 4)
    base = _keys_of(rng.normal(0.0, 1.0, N) * 10.0 ** rng.integers(-30, 30, N)).astype(np.int64)
    kind = rng.integers(0, 6, N)
    zero = np.array([0x7FFFFFFF, 0x80000000, 0x7FFFFFFE, 0x80000001], dtype=np.int64)
    base = np.where(kind == 5, zero[rng.integers(0, 4, N)], base)
    step = np.where(kind == 0, 1, np.where(kind == 1, 0, np.where(kind == 2, rng.integers(0, 5, N), rng.integers(0, 1 << 20, N))))
    a1 = base
    b1 = a1 + step * (rng.integers(0, 2, N))
    a3 = b1 + step * (rng.integers(0, 3, N))
    b3 = a3 + step * (rng.integers(0, 2, N))
    huge = kind == 4                                    # a huge gap: the extremes of fp32
    a1 = np.where(huge, int(_keys_of(np.float32(-3.4e38))[0]) + rng.integers(0, 3, N), a1)
    b3 = np.where(huge, int(_keys_of(np.float32(3.4e38))[0]) - rng.integers(0, 3, N), b3)
    b1 = np.where(huge & (rng.integers(0, 2, N) == 0), a1, b1)
    a3 = np.where(huge, np.maximum(a3, b1), a3)
    a3 = np.minimum(a3, b3)
    b1 = np.minimum(b1, a3)
    rows.append(np.stack([n, a1, b1, a3, b3]))
    out = np.concatenate(rows, axis=1)
    lim_lo, lim_hi = 0x00800000, 0xFF7FFFFF            # finite values only
    out[1:] = np.clip(out[1:], lim_lo, lim_hi)
    # (order statistics: a <= b in each pair and the pairs in order; with n == 2 both quartile ranks are 0, so b1 may exceed a3)
    assert (out[1] <= out[2]).all() and (out[3] <= out[4]).all() and (out[1] <= out[3]).all() and (out[2] <= out[4]).all() and (out[0] >= 2).all()
    return out.astype(U32)


@functools.lru_cache(maxsize=None)
def moments_cases():
    """n, n_full, lb, ub, A1, A2, T1, T2 as the step forms them from histories of fp32-valued keys: A1 = sum v, A2 = sum v^2, the tail
    corrections T1 = sum (v - bound), T2 = sum (v^2 - bound^2) over the keys beyond the bounds -- each an fp64 number the way a running
    sum would hold it (rounded sums), so the reference is the exact function of these doubles."""
    rng = np.random.default_rng(5150)
    N = 100_000
    n = rng.integers(32, HIST + 1, N)
    n[:8] = (32, 33, 34, 35, HIST, HIST - 1, HIST - 2, HIST - 3)
    scale = 10.0 ** rng.integers(-3, 5, N)
    centre = rng.normal(0.0, 1.0, N) * scale * rng.choice([0.0, 1.0, 100.0], N)      # a mean far from zero cancels in m2 - mean^2
    sd = scale * 10.0 ** rng.uniform(-4, 0, N)
    # a sample of up to 24 values stands for the history's shape; the sums are scaled to n keys
    m = 24
    v = (centre[:, None] + sd[:, None] * rng.normal(0.0, 1.0, (N, m))).astype(np.float32).astype(np.float64)
    q1, q3 = np.percentile(v, 25, axis=1), np.percentile(v, 75, axis=1)
    iqr = q3 - q1
    lb, ub = q1 - 1.5 * iqr, q3 + 1.5 * iqr
    flat = rng.integers(0, 50, N) == 0                 # iqr == 0: ub == lb
    lb = np.where(flat, q1, lb)
    ub = np.where(flat, q1, ub)
    rep = n / m
    A1 = v.sum(axis=1) * rep
    A2 = (v * v).sum(axis=1) * rep
    over, under = v > ub[:, None], v < lb[:, None]
    T1 = (np.where(over, v - ub[:, None], 0.0).sum(axis=1) + np.where(under, v - lb[:, None], 0.0).sum(axis=1)) * rep
    T2 = (np.where(over, v * v - (ub * ub)[:, None], 0.0).sum(axis=1) + np.where(under, v * v - (lb * lb)[:, None], 0.0).sum(axis=1)) * rep
    const = rng.integers(0, 40, N) == 0                # a constant history: var == 0 up to rounding
    A1 = np.where(const, centre * n, A1)
    A2 = np.where(const, centre * centre * n, A2)
    T1 = np.where(const, 0.0, T1)
    T2 = np.where(const, 0.0, T2)
    n_full = np.where(rng.integers(0, 2, N) == 0, n, rng.choice([0, HIST, 100, 257], N))
    assert np.isfinite(A1).all() and np.isfinite(A2).all() and np.isfinite(T1).all() and np.isfinite(T2).all()
    return dict(n=n.astype(np.int64), n_full=n_full.astype(np.int64), lb=lb, ub=ub, A1=A1, A2=A2, T1=T1, T2=T2)


def np_clipped_moments(C):
    """clipped_moments of sdc_trackers.hpp restated in NumPy fp64 (the algorithm without the device: the reciprocal square root from an
    fp32 seed and two Newton steps, the divisions as the correctly rounded quotient both division forms give)."""
    n = C["n"].astype(np.float64)
    C1, C2 = C["A1"] - C["T1"], C["A2"] - C["T2"]
    mean, m2 = C1 / n, C2 / n
    var = m2 - mean * mean
    pos = (var > 1e-30) & (C["ub"] > C["lb"])
    v = np.where(pos, var, 1.0)
    y = (np.float32(1.0) / np.sqrt(v.astype(np.float32))).astype(np.float64)
    hv = 0.5 * v
    for _ in range(2):
        y = y * ((-hv * y) * y + 1.5)
    return mean, np.where(pos, var * y, 0.0), np.where(pos, y, 1.0)


def check_moments(mean, sd, inv_sd, C=None, ref=None):
    """The three outputs of clipped_moments against the exact function of its inputs.  Returns the worst ratios to the two bounds."""
    C = C or moments_cases()
    rmean, rsd, rm2, rvar, pos = ref or M.moments_reference(C)
    bm = 4 * M.EPS * (np.abs(C["A1"]) + np.abs(C["T1"])) / C["n"]
    em = np.abs(mean - rmean)
    bad = ~(em <= bm)
    assert not bad.any(), ("mean", int(bad.sum()), int(np.argmax(bad)), float(mean[np.argmax(bad)]), float(rmean[np.argmax(bad)]))
    # the device decides var > 1e-30 on its rounded var: where the exact var is within its error of the threshold either answer stands
    dvar_pos = sd != 0.0
    near = np.abs(rvar - 1e-30) <= 8 * M.EPS * rm2
    flip = (dvar_pos != pos) & ~near
    assert not flip.any(), ("sd == 0 on the wrong side of var > 1e-30", int(flip.sum()), int(np.argmax(flip)))
    z = ~dvar_pos
    assert (inv_sd[z] == 1.0).all() and (sd[z] == 0.0).all()
    m = dvar_pos & pos
    bs = 8 * M.EPS * rm2[m] / rvar[m] + 1e-15
    es = np.abs(sd[m] / rsd[m] - 1.0)
    bad = ~(es <= bs)
    assert not bad.any(), ("sd", int(bad.sum()), float(es[bad].max()), float(bs[bad][np.argmax(es[bad])]))
    ei = np.abs(inv_sd[m] * rsd[m] - 1.0)
    bad = ~(ei <= bs)
    assert not bad.any(), ("inv_sd", int(bad.sum()), float(ei[bad].max()))
    return dict(mean=float((em[bm > 0] / bm[bm > 0]).max()), sd=float((es / bs).max()), inv_sd=float((ei / bs).max()), n_pos=int(m.sum()),
                n_zero=int(z.sum()))


def check_bounds(od, ou, B=None):
    """clip_bounds' five outputs over bounds_cases(): lb, ub, ctr against numpy's lerp (+-0 equal, else bit for bit); klb, kub by
    definition, after the header's clamps."""
    B = bounds_cases() if B is None else B
    _, _, lb, ub, ctr = M.bounds_from_keys(B[0].astype(np.int64), B[1], B[2], B[3], B[4])
    for name, got, want in (("lb", od[0], lb), ("ub", od[1], ub), ("ctr", od[2], ctr)):
        bad = ~M.same_value_or_bits(got, want)
        assert not bad.any(), (name, int(bad.sum()), int(np.argmax(bad)), float(got[np.argmax(bad)]), float(want[np.argmax(bad)]), B[:, np.argmax(bad)].tolist())
    klb, kub = bound_keys_by_definition(od[0], od[1])
    for name, got, want in (("klb", ou[0], klb), ("kub", ou[1], kub)):
        bad = got != want
        i = int(np.argmax(bad))
        assert not bad.any(), (name, int(bad.sum()), hex(int(got[i])), hex(int(want[i])), float(od[0][i]), float(od[1][i]), B[:, i].tolist())
