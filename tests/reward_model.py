"""A plain sorted-list model of the history-normalised reward's state (dc_rl_amd/csrc/sdc_trackers.hpp, sdc_ringpath.hpp): NumPy and the
standard library, no GPU.  TEST INFRASTRUCTURE: the reference tests/test_gpu_reward_functions.py holds the device functions to, and
tests/test_reward_probe.py holds to itself.

A history is a multiset of uint32 keys kept as a sorted list, ordered BY KEY, not by value: -0.0 and +0.0 are adjacent distinct keys of
equal value.  Nothing here emulates lanes, registers or shifts; the window rules are the ones the comments of sdc_trackers.hpp state,
written on the sorted list.
"""
from __future__ import annotations

import bisect
from fractions import Fraction

import numpy as np

KEY_NONE = 0xFFFFFFFF
WIN = 64
HIST = 10240
SMALL_N = 32
EPS = 2.0 ** -53          # unit roundoff of fp64


# ---- keys ------------------------------------------------------------------------------------------------------------------------------------
def f32_key(bits):
    """Order-preserving key of an fp32 bit pattern: negative values complemented, the others with the sign bit set."""
    b = np.asarray(bits, dtype=np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_bits(keys):
    k = np.asarray(keys, dtype=np.uint32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)


def key_of(values):
    return f32_key(np.asarray(values, dtype=np.float32).view(np.uint32))


def key_f64(keys):
    return key_bits(keys).view(np.float32).astype(np.float64)


# ---- rank windows --------------------------------------------------------------------------------------------------------------------------------
OUTCOMES = ("evict_below", "evict_above", "evict_inside", "insert_below", "insert_above", "insert_inside", "insert_inside_dropout",
            "insert_append_end", "insert_shift", "insert_shift_p0")


class Window:
    """hist: the sorted history; (r0, hi): the window lists sorted[r0 : r0 + hi].  hi == 0: no window."""

    def __init__(self, hist, r0, hi):
        self.hist = sorted(int(k) for k in hist)
        self.r0, self.hi = int(r0), int(hi)
        assert 0 <= self.hi <= WIN and (self.hi == 0 or (0 <= self.r0 and self.r0 + self.hi <= len(self.hist)))

    def keys(self):
        """The 64 keys the window must hold: the listed ranks, KEY_NONE beyond."""
        out = np.full(WIN, KEY_NONE, dtype=np.uint32)
        if self.hi > 0:
            out[:self.hi] = self.hist[self.r0:self.r0 + self.hi]
        return out

    def evict(self, y):
        """Remove one occurrence of y.  Returns (outcome, changed).  y absent but inside the window's span: the window is dropped."""
        y = int(y)
        if self.hi == 0:
            self._remove(y)
            return None, False
        first, last = self.hist[self.r0], self.hist[self.r0 + self.hi - 1]
        if y > last:                         # above the window: no rank inside it moves
            self._remove(y)
            return "evict_above", False
        if y < first:                        # below the window: every rank inside it moves down
            self._remove(y)
            self.r0 -= 1
            return "evict_below", False
        i = bisect.bisect_left(self.hist, y, self.r0, self.r0 + self.hi)
        if i >= self.r0 + self.hi or self.hist[i] != y:
            self.hi = 0                      # inside the span and not there: an inconsistent tracker is dropped
            return "inconsistent", False
        del self.hist[i]                     # inside (equal keys are interchangeable)
        self.hi -= 1
        return "evict_inside", True

    def _remove(self, y):
        i = bisect.bisect_left(self.hist, y)
        if i < len(self.hist) and self.hist[i] == y:
            del self.hist[i]

    def insert(self, x):
        """Add x.  Returns (outcome, changed)."""
        x = int(x)
        m = len(self.hist)
        if self.hi == 0:
            bisect.insort(self.hist, x)
            return None, False
        first, last = self.hist[self.r0], self.hist[self.r0 + self.hi - 1]
        ends = self.r0 + self.hi == m
        starts = self.r0 == 0
        if x < first and not starts:         # below the window: every rank inside it moves up
            bisect.insort_left(self.hist, x)
            self.r0 += 1
            return "insert_below", False
        if x >= last and not ends:           # above the window, and of keys it does not list: no rank inside it moves
            # (x goes behind its equals: the window keeps the copies of `last` it lists)
            bisect.insort_right(self.hist, x)
            return "insert_above", False
        if self.hi == WIN and ends:          # full, and it must go on ending the history: the first key drops out
            bisect.insort_right(self.hist, x)
            self.r0 += 1
            return ("insert_shift_p0" if (x < first and starts) else "insert_shift"), True
        if self.hi == WIN:                   # full: the key at the far end drops out
            bisect.insort_right(self.hist, x)
            return "insert_inside_dropout", True
        bisect.insort_right(self.hist, x)
        self.hi += 1
        return ("insert_append_end" if x >= last else "insert_inside"), True

    def update(self, x_new, x_old, has_old):
        """One step: evict x_old (if has_old), then insert x_new -- unless the eviction left no window."""
        outs, ch = [], False
        if has_old:
            o, c = self.evict(x_old)
            outs.append(o)
            ch = ch or c
        o, c = self.insert(x_new)
        outs.append(o)
        return [o for o in outs if o], ch or c

    # -- what the step asks of a window
    def resolve(self, k):
        """(ok, key at rank k, key at rank k + 1 or k if that is the last)."""
        n = len(self.hist)
        kb = k if k + 1 > n - 1 else k + 1
        ok = self.hi > 0 and k >= self.r0 and kb < self.r0 + self.hi
        return ok, (self.hist[k] if ok else 0), (self.hist[kb] if ok else 0)

    def spans(self, lo, hi_key):
        """Does the window list EVERY history key in [lo, hi_key), by the header's sufficient test?"""
        if self.hi == 0:
            return False
        n = len(self.hist)
        lo_ok = self.r0 == 0 or self.hist[self.r0] < lo
        hi_ok = self.r0 + self.hi >= n or hi_key <= self.hist[self.r0 + self.hi - 1]
        return lo_ok and hi_ok

    def lists_all_in(self, lo, hi_key):
        """The property spans() promises: every history key in [lo, hi_key) is one of the window's."""
        a, b = bisect.bisect_left(self.hist, lo), bisect.bisect_left(self.hist, hi_key)
        return a >= b or (self.hi > 0 and self.r0 <= a and b <= self.r0 + self.hi)

    def crossing(self, lo, hi_key, flip):
        """(count, exact sum v, exact sum v^2, sum |v|, sum v^2) over the window keys in [lo, hi_key), v = value of key ^ flip."""
        w = self.keys()[:self.hi]
        w = w[(w >= lo) & (w < hi_key)]
        v = key_f64(w ^ np.uint32(flip))
        return len(w), exact_sum(v), exact_sum(v * v), float(np.abs(v).sum()), float((v * v).sum())


def exact_sum(v):
    """The correctly rounded sum of finite doubles."""
    import math
    return math.fsum(float(x) for x in v)


def contract_violation(keys, r0, hi, hist):
    """None if (keys[64], r0, hi) meets the window contract against the sorted history, else a message."""
    keys = np.asarray(keys, dtype=np.uint32)
    r0, hi = int(r0), int(hi)
    if hi == 0:
        return None
    n = len(hist)
    if not (0 < hi <= WIN and 0 <= r0 and r0 + hi <= n):
        return f"r0 = {r0}, hi = {hi} do not fit a history of {n}"
    want = np.asarray(hist[r0:r0 + hi], dtype=np.uint32)
    bad = np.flatnonzero(keys[:hi] != want)
    if len(bad):
        i = int(bad[0])
        return f"key {i} is {int(keys[i]):#x}, rank {r0 + i} of the history is {int(want[i]):#x} ({len(bad)} keys differ)"
    if (keys[hi:] != KEY_NONE).any():
        return f"a key beyond hi = {hi} is not KEY_NONE"
    return None


# ---- quartiles, clip bounds, moments -------------------------------------------------------------------------------------------------------------
def quartile_ranks(n):
    return (n - 1) >> 2, (3 * (n - 1)) >> 2


def window_ranks(k, n):
    a = max(0, min(k - WIN // 2, n - WIN))
    return a, min(a + WIN - 1, n - 1)


def lerp(a, b, t):
    """numpy's _lerp (lib/function_base.py): a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5; fp64, elementwise."""
    a, b, t = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(t, dtype=np.float64)
    d = b - a
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(t >= 0.5, b - d * (1.0 - t), a + d * t)


def bounds_from_keys(n, a1, b1, a3, b3):
    """q1, q3, lb, ub, ctr (fp64 arrays) from the keys at the quartile ranks k, k + 1 of histories of n keys."""
    n = np.asarray(n, dtype=np.int64)
    t1, t3 = ((n - 1) & 3) * 0.25, ((3 * (n - 1)) & 3) * 0.25
    with np.errstate(over="ignore", invalid="ignore"):
        q1, q3 = lerp(key_f64(a1), key_f64(b1), t1), lerp(key_f64(a3), key_f64(b3), t3)
        iqr = q3 - q1
        return q1, q3, q1 - 1.5 * iqr, q3 + 1.5 * iqr, 0.5 * (q1 + q3)


def quartile_keys(hist):
    """Keys at ranks k1, k1 + 1, k3, k3 + 1 (the second of a pair is the first where the rank does not exist)."""
    n = len(hist)
    k1, k3 = quartile_ranks(n)
    return hist[k1], hist[min(k1 + 1, n - 1)], hist[k3], hist[min(k3 + 1, n - 1)]


def same_value_or_bits(got, want):
    """Elementwise: equal bits, or both zero (numpy's quartile is +0.0 where the restatement gives -0.0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return (got.view(np.uint64) == want.view(np.uint64)) | ((got == 0.0) & (want == 0.0))


def clipped_moments_exact(n, lb, ub, A1, A2, T1, T2):
    """The exact function of the doubles clipped_moments is given: mean = (A1 - T1) / n, m2 = (A2 - T2) / n, var = m2 - mean^2 as
    rationals (fractions.Fraction).  Returns (mean, sd, m2, var, pos) as floats rounded once from the exact values (sd through an
    integer square root carried to 140 bits); pos is false, and sd 0, where var <= 1e-30 or ub <= lb."""
    import math
    nn = int(n)
    mean = (Fraction(float(A1)) - Fraction(float(T1))) / nn
    m2 = (Fraction(float(A2)) - Fraction(float(T2))) / nn
    var = m2 - mean * mean
    pos = bool(var > Fraction(1e-30) and ub > lb)
    sd = 0.0
    if pos:
        p, q = var.numerator, var.denominator          # sqrt(p / q) = isqrt(p q 4^k) / (q 2^k)
        k = max(0, 140 - (p * q).bit_length() // 2)
        sd = math.isqrt((p * q) << (2 * k)) / (q << k)
    return _round(mean), sd, _round(m2), _round(var), pos


def clipped_moments_mpmath(n, lb, ub, A1, A2, T1, T2):
    """The same through mpmath at 400 bits: the check of the rational form (tests/test_reward_probe.py)."""
    import mpmath
    with mpmath.workprec(400):
        f = mpmath.mpf
        mean = (f(float(A1)) - f(float(T1))) / int(n)
        m2 = (f(float(A2)) - f(float(T2))) / int(n)
        var = m2 - mean * mean
        pos = bool(var > f(1e-30) and ub > lb)
        return float(mean), (float(mpmath.sqrt(var)) if pos else 0.0), float(m2), float(var), pos


def moments_reference(C):
    """clipped_moments_exact over the arrays of a cases dict: mean, sd, m2, var (float64 arrays) and pos (bool)."""
    N = len(C["n"])
    out = np.zeros((4, N))
    pos = np.zeros(N, dtype=bool)
    cols = [C[k].tolist() for k in ("n", "lb", "ub", "A1", "A2", "T1", "T2")]
    for i, row in enumerate(zip(*cols)):
        r = clipped_moments_exact(*row)
        out[0, i], out[1, i], out[2, i], out[3, i], pos[i] = r
    return out[0], out[1], out[2], out[3], pos


def _round(q: Fraction) -> float:
    return q.numerator / q.denominator        # (int / int is correctly rounded)


def clipped_reference(hist):
    """The normalisation's reference from a sorted key history: quartiles by numpy's lerp, lb / ub / ctr, then the clipped mean and
    population std of the fp64 values of the keys, exact up to the final rounding.  Returns a dict."""
    import mpmath
    n = len(hist)
    q1, q3, lb, ub, ctr = (float(x) for x in bounds_from_keys(n, *quartile_keys(hist)))
    v = key_f64(np.asarray(hist, dtype=np.uint32))
    c = np.clip(v, lb, ub)
    fr = [Fraction(float(x)) for x in c]
    s1, s2 = sum(fr, Fraction(0)), sum((x * x for x in fr), Fraction(0))
    mean = s1 / n
    var = s2 / n - mean * mean
    with mpmath.workprec(200):
        sd = float(mpmath.sqrt(mpmath.mpf(var.numerator) / mpmath.mpf(var.denominator))) if var > 0 else 0.0
    return dict(q1=q1, q3=q3, lb=lb, ub=ub, ctr=ctr, mean=_round(mean), sd=sd, var=_round(var), m2=_round(s2 / n))


# ---- rings -------------------------------------------------------------------------------------------------------------------------------------
def ring_history(ring, patch_slot=-1, patch_x=0):
    """The sorted history a ring holds (KEY_NONE slots are empty), with the patched slot's content replaced."""
    r = np.array(ring, dtype=np.uint32, copy=True)
    if patch_slot >= 0:
        r[patch_slot] = np.uint32(patch_x)
    return np.sort(r[r != KEY_NONE])


def refill_ahead(r0, hi, k_next, n, m_lo, m_hi):
    """qt_refill_ahead: 0 none, 1 up, 2 down."""
    if hi <= 0:
        return 0
    t = k_next - r0
    if t > hi - m_hi and r0 + hi < n:
        return 1
    if t < m_lo and r0 > 0:
        return 2
    return 0
