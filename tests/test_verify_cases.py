"""tests/verify_cases.py on a small synthetic reward state, without a GPU: sorted rings with known windows, sums and counts.  The
preconditions hold, each kind changes exactly the words it names, and a ring in which a kind's precondition cannot hold is refused
(the env stays a control and is listed).  The corruptions on a real state, against the verify kernel: tests/test_gpu_verify_fires.py."""
import numpy as np
import pytest

from dc_rl_amd import _lib as L
from tests import verify_cases as VC
from tests.gpu_helpers import hdr_offsets

STRIDE = 1024


@pytest.fixture(scope="module")
def H():
    import os
    return VC.offsets(hdr_offsets(), open(os.path.join(L.CSRC, "sdc_device.hpp")).read())


def build_state(vals, H):
    """(header row, windows [64][4], ring row) of a reward state that describes the ring `vals` (fp32), as a rebuild leaves it: windows
    of up to 64 keys centred on the quartile ranks and on the first key beyond each clip bound, total and tail sums, cached keys"""
    vals = np.asarray(vals, dtype=np.float32)
    ring = np.sort(VC.f32_key(vals))
    n = len(ring)
    v = VC.key_f64(ring)
    q1, q3 = np.percentile(v, [25, 75])
    lb, ub = q1 - 1.5 * (q3 - q1), q3 + 1.5 * (q3 - q1)
    lbf, ubf = np.float32(lb), np.float32(ub)
    klb = int(VC.f32_key(lbf)[0]) + (1 if float(lbf) < lb else 0)      # the smallest key whose value is >= lb
    kub = int(VC.f32_key(ubf)[0]) + (1 if float(ubf) <= ub else 0)     # the smallest key whose value is > ub
    up, lo = ring >= kub, ring < klb
    hdr = np.zeros(64, dtype=np.uint32)
    qw = np.full((VC.WIN, 4), VC.KEY_NONE, dtype=np.uint32)
    k1, k3 = VC.quartile_ranks(n)
    for w, centre in enumerate((k1, k3, n - int(up.sum()), n - int(lo.sum()))):
        s = VC.space(ring, w)
        hi = min(VC.WIN, n)
        r0 = min(max(centre - VC.WIN // 2, 0), n - hi)
        qw[:hi, w] = s[r0:r0 + hi]
        hdr[H[VC.WINDOWS[w]] + H["T_R0"]], hdr[H[VC.WINDOWS[w]] + H["T_HI"]] = r0, hi
        hdr[H["H_WFIRST"] + w], hdr[H["H_WLAST"] + w] = s[r0], s[r0 + hi - 1]
    hdr[H["H_N"]], hdr[H["H_VALID"]] = n, 1
    hdr[H["H_KB"]], hdr[H["H_KB"] + 1] = kub, ~np.uint32(klb - 1)
    hdr[H["H_QC"]], hdr[H["H_QC"] + 1] = up.sum(), lo.sum()
    VC.put_f64(hdr, H["H_A1"], v.sum())
    VC.put_f64(hdr, H["H_A2"], (v * v).sum())
    VC.put_f64(hdr, H["H_QS1"], v[up].sum())
    VC.put_f64(hdr, H["H_QS1"] + 2, v[lo].sum())
    VC.put_f64(hdr, H["H_QS2_HI"], (v[up] ** 2).sum())
    VC.put_f64(hdr, H["H_QS2_LO"], (v[lo] ** 2).sum())
    row = np.full(STRIDE, np.nan, dtype=np.float32)
    row[:n] = vals
    return hdr, qw, row


def spread_ring(n, rng):
    """n distinct fp32 values around 331 with both tails populated, no two within two keys of each other"""
    v = np.unique((331 + 70 * rng.standard_normal(4 * n)).astype(np.float32))
    v = v[np.concatenate([[True], np.diff(VC.f32_key(v).astype(np.int64)) > 2])]
    v = rng.permutation(v)[:n - 6]
    return np.concatenate([v, np.float32([20, 30, 40, 700, 710, 720])])


def batch(H, sizes, seed=1):
    rng = np.random.default_rng(seed)
    rows = [build_state(spread_ring(n, rng), H) for n in sizes]
    return tuple(np.stack(x) for x in zip(*rows))


def changed_words(res, header, qwin, e):
    got = [("header", int(i)) for i in np.flatnonzero(res.header[e] != header[e])]
    got += [("qwin", int(p), int(w)) for p, w in np.argwhere(res.qwin[e] != qwin[e])]
    return sorted(got)


def test_the_synthetic_state_describes_its_ring(H):
    header, qwin, hist = batch(H, [33, 64, 65, 200, 1000])
    for e in range(len(header)):
        assert VC.state_fault(header[e], qwin[e], VC.ring_keys(hist[e]), H) is None, e


def test_every_kind_is_placed_with_its_preconditions_and_changes_the_words_it_names(H):
    sizes = [200] * 16 + [1000] * 16 + [70] * 16
    header, qwin, hist = batch(H, sizes)
    h0, q0 = header.copy(), qwin.copy()
    res = VC.corrupt(header, qwin, hist, H)
    assert np.array_equal(header, h0) and np.array_equal(qwin, q0)      # (the inputs are not written)
    assert res.demoted == [], res.demoted
    assert np.array_equal(res.kind, np.arange(len(sizes)) % 16)
    for e in range(len(sizes)):
        kind, ring, n = int(res.kind[e]), VC.ring_keys(hist[e]), sizes[e]
        assert res.cls[e] == VC.CLASS_OF_KIND[kind]
        words = changed_words(res, header, qwin, e)
        assert words == sorted(res.words.get(e, [])), (e, kind)
        hr, old = res.header[e], header[e]
        k1, k3 = VC.quartile_ranks(n)
        expect = {0: [], 8: [], 1: [H["H_A1"]], 2: [H["H_A2"]], 3: [H["H_QC"]], 4: [H["H_QC"] + 1], 5: [H["H_QS1"]],
                  11: [H["H_Q1"] + H["T_R0"]], 12: [H["H_Q3"] + H["T_HI"]], 13: [H["H_VALID"]], 15: [H["H_KB"]]}
        if kind in expect:      # the header words a kind names (an f64: either of its two dwords, nothing else), no window key
            assert all(wd[0] == "header" for wd in words)
            allowed = {i for b in expect[kind] for i in ((b, b + 1) if kind in (1, 2, 5) else (b,))}
            assert {wd[1] for wd in words} <= allowed and (words or kind in (0, 8)), (e, kind, words)
        if kind == 1:
            s1 = VC.key_f64(ring).sum()
            d = VC.get_f64(hr, H["H_A1"]) - VC.get_f64(old, H["H_A1"])
            assert d >= 100 * 1e-9 * (abs(s1) + n) and np.isclose(d, res.delta[e])
        if kind == 2:
            assert np.isclose(VC.get_f64(hr, H["H_A2"]) - VC.get_f64(old, H["H_A2"]), n * VC.clipped_moments(ring)[1] ** 2)
        if kind == 3:
            assert int(hr[H["H_QC"]]) == int(old[H["H_QC"]]) + 1
        if kind == 4:
            assert int(hr[H["H_QC"] + 1]) == int(old[H["H_QC"] + 1]) - 1 >= 0
        if kind == 5:
            d = VC.get_f64(hr, H["H_QS1"]) - VC.get_f64(old, H["H_QS1"])
            assert d / (n * VC.clipped_moments(ring)[1]) >= 100 * (2e-6 * 50 + 1e-6) - 1e-12
        if kind in (6, 7, 9, 10):
            (_, p, w), = words
            assert w == {6: 0, 7: 1, 9: 2, 10: 3}[kind]
            keys, r0, hi = VC.window(old, qwin[e], w, H)
            new = int(res.qwin[e, p, w])
            flip = VC.KEY_NONE if w == 3 else 0
            assert new == int(keys[p]) + 1 and 0 < p < hi - 1 and int(keys[p - 1]) < new < int(keys[p + 1])
            assert (new ^ flip) not in ring
            if kind == 7:
                assert p == k3 - r0
            if kind == 6:
                assert abs(p - (k1 - r0)) >= 2
        if kind == 11:
            assert int(hr[H["H_Q1"] + H["T_R0"]]) == int(old[H["H_Q1"] + H["T_R0"]]) + 1
            assert len({int(ring[k1]), int(ring[k1 + 1]), int(ring[k1 + 2])}) == 3
        if kind == 12:
            assert int(hr[H["H_Q3"] + H["T_HI"]]) == 0
        if kind == 13:
            assert int(hr[H["H_VALID"]]) == 0
        if kind == 14:
            (_, i), = words
            assert H["H_WFIRST"] <= i < H["H_WFIRST"] + 4 and abs(int(hr[i]) - int(old[i])) == 1
        if kind == 15:
            keys = VC.window(old, qwin[e], 2, H)[0]
            assert int(hr[H["H_KB"]]) in keys.tolist() and int(hr[H["H_KB"]]) != int(old[H["H_KB"]])
            assert abs(int((keys < hr[H["H_KB"]]).sum()) - int((keys < old[H["H_KB"]]).sum())) == 1      # over ONE window key
        # what no kind may touch: lengths, stamps, the previous step's keys
        for name, cnt in (("H_N", 1), ("H_PEND", 4), ("H_LAST_XNEW", 1), ("H_LAST_XOLD", 1), ("H_LAST_NPREV", 1)):
            assert np.array_equal(hr[H[name]:H[name] + cnt], old[H[name]:H[name] + cnt])
        # the consistency the verify kernel's checks 1 and 3 ask for is what the rank / count / total corruptions break
        fault = VC.state_fault(res.header[e], res.qwin[e], ring, H)
        if kind in (1, 3, 4, 6, 7, 9, 10, 11, 12, 13, 14, 15):
            assert fault is not None, (e, kind)
        if kind in (0, 8, 2, 5):      # (A2 and the tail sums are held by the z check alone)
            assert fault is None, (e, kind, fault)


def one_env(H, vals, env):
    """a batch of env + 1 envs whose last env holds the ring `vals`: its kind is env % 16"""
    rng = np.random.default_rng(5)
    rows = [build_state(spread_ring(100, rng), H) for _ in range(env)] + [build_state(vals, H)]
    header, qwin, hist = (np.stack(x) for x in zip(*rows))
    res = VC.corrupt(header, qwin, hist, H)
    return res, header, qwin


def test_a_ring_in_which_a_precondition_cannot_hold_is_refused(H):
    rng = np.random.default_rng(9)
    base = np.sort(spread_ring(200, rng))
    n = len(base)
    k1, k3 = VC.quartile_ranks(n)
    # kind 7: a duplicate at the upper quartile
    v = base.copy()
    v[k3 + 1] = v[k3]
    res, header, qwin = one_env(H, v, 7)
    assert res.demoted == [(7, 7, "the key at the quartile rank has no room above it (a duplicate, a neighbour one key up, the window's end)")]
    assert res.kind[7] == 0 and res.cls[7] == VC.CLEAN
    assert np.array_equal(res.header[7], header[7]) and np.array_equal(res.qwin[7], qwin[7])
    # kind 7: the new key is in the ring already (the next key up)
    v = base.copy()
    v[k3 + 1] = np.nextafter(v[k3], np.float32(np.inf))
    res, header, qwin = one_env(H, v, 7)
    assert [d[:2] for d in res.demoted] == [(7, 7)] and np.array_equal(res.qwin[7], qwin[7])
    # kind 11: duplicates at the lower quartile
    v = base.copy()
    v[k1 + 2] = v[k1 + 1]
    res, header, qwin = one_env(H, v, 11)
    assert res.demoted == [(11, 11, "the keys at ranks k1, k1 + 1, k1 + 2 are not pairwise different")]
    assert np.array_equal(res.header[11], header[11])
    # kind 4: no key below the lower bound
    v = base[(base > 200) & (base < 460)]
    res, header, qwin = one_env(H, v, 4)
    assert res.demoted == [(4, 4, "no key below the lower bound: the count would go negative")]
    # kind 6: a window whose every interior key has its successor in the ring (consecutive keys)
    k0 = int(VC.f32_key(np.float32(331.0))[0])
    dense = VC.key_f64(np.arange(k0, k0 + 80, dtype=np.uint32)).astype(np.float32)
    res, header, qwin = one_env(H, dense, 6)
    assert res.demoted == [(6, 6, "no interior key with room above it")]
    # a state that does not describe its ring is not corrupted further
    hdr, qw, row = build_state(base, H)
    hdr[H["H_QC"]] += 1
    res = VC.corrupt(hdr[None], qw[None], row[None], H)
    assert res.demoted == [] and res.kind[0] == 0      # (env 0 is a control: nothing is asked of its state)
    header, qwin, hist = np.stack([hdr] * 2), np.stack([qw] * 2), np.stack([row] * 2)
    res = VC.corrupt(header, qwin, hist, H)
    assert res.demoted == [(1, 1, "the state does not describe the ring: H_QC is not the ring's tail counts")]


def test_an_env_below_small_n_is_clean_whatever_was_written(H):
    """31 keys: no reward state (windows of 0 keys, H_VALID 0) -- the scalar kinds are still written, the class is `clean`"""
    rng = np.random.default_rng(3)
    rows = []
    for _ in range(16):
        vals = spread_ring(31, rng)
        hdr, qw, row = build_state(np.concatenate([vals, np.float32([331.5])]), H)      # (a state of 32 keys, taken apart below)
        row[31] = np.nan
        for w in range(4):
            hdr[H[VC.WINDOWS[w]] + H["T_HI"]] = 0
        qw[:] = VC.KEY_NONE
        hdr[H["H_N"]], hdr[H["H_VALID"]] = 31, 0
        rows.append((hdr, qw, row))
    header, qwin, hist = (np.stack(x) for x in zip(*rows))
    res = VC.corrupt(header, qwin, hist, H)
    assert (res.cls == VC.CLEAN).all() and (res.n == 31).all()
    assert {k for _, k, _ in res.demoted} >= {6, 7, 9, 10, 12, 13, 14, 15}      # (nothing to corrupt in a window that is not there)
    assert res.kind[1] == 1 and res.kind[3] == 3 and np.array_equal(res.qwin, qwin)
