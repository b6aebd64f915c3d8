"""Scripted corruptions of a REAL reward state, for the tests that show verify mode firing (csrc/sdc_verify.hip, debug_flags bit 0;
tests/test_gpu_verify_fires.py on the device, tests/test_verify_cases.py on a synthetic state without one).  NumPy only.

In: the arrays as `get_state` returns them -- `header` uint32 [N][64], `qwin` uint32 [N][64][4] (lane l's keys of {Q1, Q3, BU, BL}),
`hist` float32 [N][stride] (NaN: empty slot) -- and the dword names (`offsets()`: enum SdcHdr / SdcTrack of csrc/sdc_device.hpp, never a
literal number).  Out: corrupted COPIES of header and qwin and, per env, the kind that was placed and the class expected of it.

Kinds go by env % 16, so every wavefront of every mapping mixes corrupted and clean envs, and in the kernels with two envs per
wavefront every corrupted env sits beside a clean one (the fault must land in the right info row):

  kind  corruption                                                  class
  0, 8  none (control)                                              clean
  1     H_A1 += d,  d = 1000 x the verify kernel's tolerance        must fire   (check 3: running total)
  2     H_A2 += n x (clipped variance of the ring)                  must fire   (check 2: sd grows by sqrt 2, z with it)
  3     H_QC[0] += 1                                                must fire   (check 3: tail count)
  4     H_QC[1] -= 1   (needs a key below the lower bound)          must fire
  5     H_QS1 upper += 0.02 n sd    (z moves by 0.02)               must fire   (check 2)
  6     Q1 window: an interior key + 1, away from the quartile      must fire   (check 1: every window key against its rank)
  7     Q3 window: the key at the resolved quartile rank + 1        must fire   (check 1: rank, bisection)
  9     BU window: an interior key + 1                              must fire
  10    BL window (complemented keys): an interior key + 1          must fire
  11    H_Q1 + T_R0 += 1                                            must fire   (check 1: bisection, ranks)
  12    H_Q3 + T_HI = 0                                             healed      (no window: the step rebuilds from the ring)
  13    H_VALID = 0                                                 healed
  14    one H_WFIRST word +- 1                                      either      (a key landing inside the window rewrites the cache)
  15    H_KB[0] moved over the neighbouring key of the BU window    either

An env below SMALL_N keys has no reward state (the step works from the ring, the verify kernel returns early): its class is `clean`
whatever was written into its header.

PRECONDITIONS, asserted per env before anything is written (a kind whose precondition cannot hold is NOT placed: the env becomes a
control and is listed in `Result.demoted` with the reason):
  * the state describes the ring to begin with: VALID, four windows, every window key at its rank, A1 within the kernel's tolerance;
  * a new window key is not in the ring (x ^ flip for BL), lies strictly between its neighbours, is not the window's first or last;
  * d is at least 100 x the verify kernel's own tolerance for that env (H_A1: 1e-9 (|sum| + n), the sum taken from the ring here;
    z: 2e-6 |z| + 1e-6, good for |z| < 50);
  * kind 11: the keys at ranks k1, k1 + 1, k1 + 2 are pairwise different.

SAFETY: a corruption changes values and ranks only -- never an index, a length or a stamp that a kernel turns into an address or a loop
bound (H_PEND, H_N, H_LAST_*, hist_len, hist_pos are left alone; T_R0 moves by 1; T_HI is set to 0, "no window", and to nothing else).
What was read for it (csrc/sdc_pairstep.hpp, sdc_halfwin.hpp, sdc_quadwin.hpp, sdc_ringpath.hpp, sdc_wide.hip): r0, hi and the counts
enter comparisons, rank arithmetic and lane selects (readlane / bpermute: six bits of lane); the lane-per-env kernel's window positions
cb[] are clamped to 0 .. 63 before they index qwin; a re-centring request carries r0 / hi / the wanted rank into qt_refill, where the
rank only sets how many lanes are dropped (clamped to 0 .. hi - 1) and every LDS position is guarded by `< WIN`."""
import re

import numpy as np

SMALL_N = 32           # csrc/sdc_trackers.hpp
WIN = 64               # SDC_WIN
KEY_NONE = 0xFFFFFFFF
WINDOWS = ("H_Q1", "H_Q3", "H_BU", "H_BL")      # window order of qwin's last axis, of H_WFIRST / H_WLAST
CLEAN, MUST_FIRE, HEALED, EITHER = "clean", "must fire", "healed", "either"
CLASS_OF_KIND = {0: CLEAN, 8: CLEAN, 12: HEALED, 13: HEALED, 14: EITHER, 15: EITHER,
                 **{k: MUST_FIRE for k in (1, 2, 3, 4, 5, 6, 7, 9, 10, 11)}}
NAME_OF_KIND = {0: "control", 8: "control", 1: "A1 += d", 2: "A2 += n var", 3: "QC[0] += 1", 4: "QC[1] -= 1", 5: "QS1 upper += d",
                6: "Q1 interior key + 1", 7: "Q3 quartile key + 1", 9: "BU interior key + 1", 10: "BL interior key + 1",
                11: "Q1 r0 += 1", 12: "Q3 hi = 0", 13: "VALID = 0", 14: "WFIRST +- 1", 15: "KB[0] over a key"}
A1_TOL = 1e-9          # sdc_verify.hip check 3: |sum - A1| <= 1e-9 (|sum| + n)


def z_tol(z):
    """sdc_verify.hip check 2"""
    return 2e-6 * np.abs(z) + 1e-6


def offsets(hdr_offsets, device_hpp_text):
    """hdr_offsets (tests/gpu_helpers.hdr_offsets()) with T_R0 / T_HI of enum SdcTrack added"""
    body = re.search(r"enum SdcTrack \{(.*?)\};", device_hpp_text, re.S)
    assert body, "enum SdcTrack not found in sdc_device.hpp"
    H = dict(hdr_offsets)
    H.update({m.group(1): int(m.group(2)) for m in re.finditer(r"\b(T_\w+)\s*=\s*(\d+)", body.group(1))})
    assert {"T_R0", "T_HI"} <= set(H)
    return H


# ---- keys (csrc/sdc_trackers.hpp f32_key / key_f32) ----------------------------------------------------------------------------------
def f32_key(f):
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def key_f64(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    b = np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k)
    return b.view(np.float32).astype(np.float64)


def ring_keys(hist_row):
    """sorted keys of one env's ring (NaN: empty slot)"""
    v = np.asarray(hist_row, dtype=np.float32)
    return np.sort(f32_key(v[~np.isnan(v)]))


def get_f64(row, i):
    return float(np.array(row[i:i + 2], dtype=np.uint32).view(np.float64)[0])


def put_f64(row, i, v):
    row[i:i + 2] = np.array([v], dtype=np.float64).view(np.uint32)


def quartile_ranks(n):
    return (n - 1) >> 2, (3 * (n - 1)) >> 2


def clipped_moments(ring):
    """(mean, sd) of the ring clipped to q -+ 1.5 iqr (np.percentile, linear): utils/reward_creator.py:16-45 in fp64"""
    v = key_f64(ring)
    q1, q3 = np.percentile(v, [25, 75])
    c = np.clip(v, q1 - 1.5 * (q3 - q1), q3 + 1.5 * (q3 - q1))
    return float(c.mean()), float(c.std())


def z_reference(hist_row, e_off):
    """the z-score the step reports, from the ring as read back AFTER the step and the header's H_EOFF"""
    m, sd = clipped_moments(ring_keys(hist_row))
    return (e_off - m) / (sd if sd > 0 else 1.0)


# ---- the state's own consistency ------------------------------------------------------------------------------------------------------
def window(header_row, qwin_env, w, H):
    """(keys [hi] in the window's own key space, r0, hi)"""
    base = H[WINDOWS[w]]
    r0, hi = int(np.int32(header_row[base + H["T_R0"]])), int(np.int32(header_row[base + H["T_HI"]]))
    return qwin_env[:max(hi, 0), w].copy(), r0, hi


def space(ring, w):
    """the ring's keys, sorted, in window w's key space (BL: complemented)"""
    return np.sort(~ring) if w == 3 else ring


def state_fault(header_row, qwin_env, ring, H):
    """None if the reward state describes the ring the way the verify kernel's checks 1 and 3 ask, else what does not"""
    n = int(header_row[H["H_N"]])
    if n != len(ring):
        return f"H_N {n} but {len(ring)} keys in the ring"
    if int(header_row[H["H_VALID"]]) != 1:
        return "H_VALID is not 1"
    for w in range(4):
        keys, r0, hi = window(header_row, qwin_env, w, H)
        if not (0 < hi <= WIN and r0 >= 0 and r0 + hi <= n):
            return f"window {w}: r0 {r0} hi {hi} n {n}"
        s = space(ring, w)
        rank = r0 + np.arange(hi)
        if not (np.all(np.searchsorted(s, keys, "left") <= rank) and np.all(rank < np.searchsorted(s, keys, "right"))):
            return f"window {w}: a key is not at its rank"
        if (qwin_env[hi:, w] != KEY_NONE).any():
            return f"window {w}: a key beyond hi"
        if int(header_row[H["H_WFIRST"] + w]) != int(keys[0]) or int(header_row[H["H_WLAST"] + w]) != int(keys[-1]):
            return f"window {w}: cached first / last key"
    s1 = float(key_f64(ring).sum())
    if not abs(s1 - get_f64(header_row, H["H_A1"])) <= A1_TOL * (abs(s1) + n):
        return "H_A1 is not the ring's sum"
    kb0, kb1 = int(header_row[H["H_KB"]]), int(header_row[H["H_KB"] + 1])
    if int(header_row[H["H_QC"]]) != int((ring >= kb0).sum()) or int(header_row[H["H_QC"] + 1]) != int((~ring >= kb1).sum()):
        return "H_QC is not the ring's tail counts"
    return None


def interior_slot(keys, s, avoid=(), want=None):
    """a window position p, 0 < p < hi - 1, whose key + 1 lies strictly below the next key and is not in the ring (`s`: the ring in the
    window's key space): `want` itself, or the admissible one nearest the window's middle outside `avoid`.  None: there is none."""
    hi = len(keys)
    k = keys.astype(np.int64)
    ok = np.zeros(hi, dtype=bool)
    if hi >= 3:
        ok[1:-1] = (k[1:-1] + 1 < k[2:]) & (k[:-2] < k[1:-1] + 1)
    ok &= ~np.isin(k + 1, s.astype(np.int64))
    for p in avoid:
        if 0 <= p < hi:
            ok[p] = False
    if want is not None:
        return want if 0 <= want < hi and ok[want] else None
    cand = np.flatnonzero(ok)
    return int(cand[np.argmin(np.abs(cand - hi // 2))]) if len(cand) else None


class Result:
    """header, qwin: the corrupted copies.  kind [N]: the kind placed (0 where it could not be); wanted [N]: env % 16; cls [N]: the
    class expected; demoted: [(env, wanted kind, reason)]; words: {env: [("header" | "qwin", index...)]} the words a kind changed;
    delta: {env: d} for the kinds that add one."""

    def __init__(self, header, qwin, N):
        self.header, self.qwin = header, qwin
        self.wanted = np.arange(N) % 16
        self.kind = np.zeros(N, dtype=np.int64)
        self.cls = np.array([CLEAN] * N, dtype=object)
        self.demoted, self.words, self.delta, self.n = [], {}, {}, np.zeros(N, dtype=np.int64)

    def envs(self, cls=None, kind=None):
        m = np.ones(len(self.kind), dtype=bool)
        if cls is not None:
            m &= self.cls == cls
        if kind is not None:
            m &= self.kind == kind
        return np.flatnonzero(m)


def place(kind, hrow, qenv, ring, H):
    """Corrupt one env's header row / windows IN PLACE for `kind`.  Returns (words changed, d or None), or a string: why the kind's
    precondition cannot hold (nothing was written)."""
    n = len(ring)
    small = n < SMALL_N
    if not small:
        bad = state_fault(hrow, qenv, ring, H)
        if bad:
            return "the state does not describe the ring: " + bad
    k1, k3 = quartile_ranks(n)
    hdr = lambda *idx: [("header", int(i)) for i in idx]
    if kind in (1, 2, 5):
        if n < 2:
            return "fewer than two keys"
        mean, sd = clipped_moments(ring)
        s1 = float(key_f64(ring).sum())
        i, d = {1: (H["H_A1"], 1000.0 * A1_TOL * (abs(s1) + n)), 2: (H["H_A2"], n * sd * sd), 5: (H["H_QS1"], 0.02 * n * sd)}[kind]
        if not d > 0:
            return "a ring without spread"
        if kind == 1:
            assert d >= 100 * A1_TOL * (abs(s1) + n)
        if kind == 5:      # z moves by d / (n sd) = 0.02 (the mean's share alone)
            assert d / (n * sd) >= 100 * z_tol(50.0) - 1e-15
        v = get_f64(hrow, i)
        if not (v + d != v and np.isfinite(v + d)):
            return "the sum would not change"
        put_f64(hrow, i, v + d)
        return hdr(i, i + 1), d
    if kind == 3:
        hrow[H["H_QC"]] += 1
        return hdr(H["H_QC"]), None
    if kind == 4:
        if int(np.int32(hrow[H["H_QC"] + 1])) < 1:
            return "no key below the lower bound: the count would go negative"
        hrow[H["H_QC"] + 1] -= 1
        return hdr(H["H_QC"] + 1), None
    if kind in (6, 7, 9, 10):
        w = {6: 0, 7: 1, 9: 2, 10: 3}[kind]
        keys, r0, hi = window(hrow, qenv, w, H)
        if small or hi <= 0:
            return "no window"
        s = space(ring, w)
        if kind == 7:
            p = interior_slot(keys, s, want=k3 - r0)
            why = "the key at the quartile rank has no room above it (a duplicate, a neighbour one key up, the window's end)"
        else:
            t = k1 - r0
            p = interior_slot(keys, s, avoid=(t - 1, t, t + 1, t + 2) if kind == 6 else ())
            why = "no interior key with room above it"
        if p is None:
            return why
        new = int(keys[p]) + 1
        assert 0 < p < hi - 1 and int(keys[p - 1]) < new < int(keys[p + 1]) and new not in s      # (s: already in the window's key space)
        qenv[p, w] = new
        return [("qwin", p, w)], None
    if kind == 11:
        if k1 + 2 >= n or len({int(ring[k1]), int(ring[k1 + 1]), int(ring[k1 + 2])}) != 3:
            return "the keys at ranks k1, k1 + 1, k1 + 2 are not pairwise different"
        i = H["H_Q1"] + H["T_R0"]
        hrow[i] += 1
        return hdr(i), None
    if kind == 12:
        i = H["H_Q3"] + H["T_HI"]
        if int(hrow[i]) == 0:
            return "no window to drop"
        hrow[i] = 0
        return hdr(i), None
    if kind == 13:
        if int(hrow[H["H_VALID"]]) == 0:
            return "not valid to begin with"
        hrow[H["H_VALID"]] = 0
        return hdr(H["H_VALID"]), None
    if kind in (14, 15) and small:
        return "no window"
    if kind == 14:
        return None      # (placed by the caller: which word and which sign go by the env)
    if kind == 15:
        keys, r0, hi = window(hrow, qenv, 2, H)
        kb0 = int(hrow[H["H_KB"]])
        pos = int((keys.astype(np.int64) < kb0).sum())      # the first window key at or beyond the bound
        if pos + 1 < hi and int(keys[pos + 1]) > int(keys[pos]):
            new = int(keys[pos + 1])                        # up: the key at `pos` leaves the tail
        elif pos >= 1 and int(keys[pos - 1]) < kb0 and (pos < 2 or int(keys[pos - 2]) < int(keys[pos - 1])):
            new = int(keys[pos - 1])                        # down: the key at `pos - 1` enters it
        else:
            return "the bound has no neighbouring key in the window"
        if new == kb0:
            return "the bound sits on that key already"
        hrow[H["H_KB"]] = new
        return hdr(H["H_KB"]), None
    raise AssertionError(kind)


def corrupt(header, qwin, hist, H):
    """-> Result.  header / qwin / hist as get_state returns them (not modified)."""
    header = np.array(header, dtype=np.uint32, copy=True)
    qwin = np.array(qwin, dtype=np.uint32, copy=True)
    N = len(header)
    assert header.shape == (N, 64) and qwin.shape == (N, WIN, 4)
    out = Result(header, qwin, N)
    for e in range(N):
        kind = int(out.wanted[e])
        ring = ring_keys(hist[e])
        out.n[e] = len(ring)
        assert int(header[e, H["H_N"]]) == len(ring), (e, int(header[e, H["H_N"]]), len(ring))
        if CLASS_OF_KIND[kind] == CLEAN:
            out.kind[e] = kind
            continue
        hrow, qenv = header[e].copy(), qwin[e].copy()
        got = place(kind, hrow, qenv, ring, H)
        if got is None:      # kind 14
            w = (e // 16) % 4
            i = H["H_WFIRST"] + w
            v = int(hrow[i]) + (1 if (e // 64) % 2 == 0 else -1)
            got = "the cached key would wrap" if not 0 < v < KEY_NONE - 1 else ([("header", i)], None)
            if not isinstance(got, str):
                hrow[i] = v
        if isinstance(got, str):
            out.demoted.append((e, kind, got))
            continue
        header[e], qwin[e] = hrow, qenv
        out.kind[e] = kind
        out.words[e], d = got
        if d is not None:
            out.delta[e] = d
        out.cls[e] = CLEAN if len(ring) < SMALL_N else CLASS_OF_KIND[kind]
    return out
