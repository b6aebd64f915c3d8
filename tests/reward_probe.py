"""Build and drive tests/aux/reward_probe.hip: the history-normalised reward's device code (dc_rl_amd/csrc/sdc_trackers.hpp,
sdc_halfwin.hpp, sdc_quadwin.hpp, sdc_ringpath.hpp), one function per kernel and one case per workgroup.

TEST INFRASTRUCTURE ONLY.  Built with the library's own flags by the code tests/physics_probe.py uses (tests/probe_build.py);
__graft_entry__.build() builds it beside the physics probe.  The buffer layouts are the ones tests/aux/reward_probe.hip states at each
kernel; integers travel as 32-bit words, keys as uint32.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests.probe_build import OUT_DIR, ROOT, Probe      # noqa: F401

LAUNCHERS = {            # launcher -> number of pointer arguments (then the case count(s) and the stream)
    "keys": 2, "reduce": 4, "window_ops_qtrack": 7, "window_ops_hwin": 7, "window_ops_qwin": 7, "bounds": 3, "moments": 3,
    "refill5": 5, "refill10": 5, "refill_coop": 5, "rebuild": 5, "bisect_build": 5,
}
FORMS = {"QTrack": ("window_ops_qtrack", 1), "HWin": ("window_ops_hwin", 2), "QWin": ("window_ops_qwin", 4)}   # launcher, slots per wavefront
HIST = 10240             # SDC_HIST_STRIDE
COOP_NW = 4
# oi columns of window_ops
OI = dict(r0=0, hi=1, ch=2, ok1=3, a1=4, b1=5, ok3=6, a3=7, b3=8, span0=9, span1=10, any0=11, c0=12, any1=13, c1=14, first=15, last=16, n=17)
OI_W = 20
NOT_APPLICABLE = 2

_PROBE = Probe("reward_probe", "reward probe")
SRC, LIB_PATH, BUILD_HINT = _PROBE.src, _PROBE.lib_path, _PROBE.build_hint
build_command, build = _PROBE.build_command, _PROBE.build


def _declare(lib):
    for name, n_ptr in LAUNCHERS.items():
        fn = getattr(lib, "probe_" + name)
        n_int = 2 if name.startswith("window_ops") else 1
        fn.argtypes = [C.c_void_p] * n_ptr + [C.c_int] * n_int + [C.c_void_p]
        fn.restype = C.c_int


def load():
    """The loaded probe.  A missing probe is an error that names the build command: the GPU machine runs what build() made."""
    return _PROBE.load(_declare)


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    assert a.dtype in (np.int32, np.float64), a.dtype
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def _out(shape, kind):
    import torch
    dev = torch.device("cuda", 0)
    if kind == "f64":
        return torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    return torch.full(shape, -0x21524111, dtype=torch.int32, device=dev)      # (a pattern no case produces: an unwritten word shows)


def _back(t, kind):
    a = t.cpu().numpy()
    return a.view(np.uint32) if kind == "u32" else a


def _launch(name, ins, outs, *counts):
    """ins: NumPy arrays; outs: [(shape, 'u32' | 'i32' | 'f64')]; returns the outputs as NumPy arrays."""
    import torch
    lib = load()
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        din = [_to_dev(a) for a in ins]
        dout = [_out(s, k) for s, k in outs]
        rc = getattr(lib, "probe_" + name)(*[t.data_ptr() for t in din + dout], *[int(c) for c in counts],
                                            torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"probe_{name}: hipError {rc}"
        torch.cuda.synchronize()
    return [_back(t, k) for t, (_, k) in zip(dout, outs)]


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def keys(bits):
    """fp32 bit patterns [n] -> (f32_key, bits of key_f32(f32_key))."""
    bits = _u32(bits)
    (o,) = _launch("keys", [bits], [((2, len(bits)), "u32")], len(bits))
    return o[0], o[1]


def reduce(u, d):
    """u [n][64] uint32, d [n][64] float64 -> dict of per-lane results [n][64]."""
    u, d = _u32(u), np.ascontiguousarray(d, dtype=np.float64)
    n = len(u)
    ou, od = _launch("reduce", [u, d], [((n, 5, 64), "u32"), ((n, 3, 64), "f64")], n)
    return dict(wave_sum_u32=ou[:, 0], wave_min_u32=ou[:, 1], wave_max_u32=ou[:, 2], half_sum_u32=ou[:, 3], row_sum_u32=ou[:, 4],
                wave_sum_f64=od[:, 0], half_sum_f64=od[:, 1], row_sum_f64=od[:, 2])


def window_ops(form, keys0, meta, ops, iv):
    """keys0 [S][64], meta [S][4] = r0, hi, n0, on, ops [S][T][4] = x_new, x_old, has_old, 0, iv [S][T][4] = lo0, hi0, lo1, hi1
    -> (keys [S][T][64], oi [S][T][OI_W], od [S][T][4])."""
    name, _ = FORMS[form]
    keys0, meta, ops, iv = _u32(keys0), _i32(meta), _u32(ops), _u32(iv)
    S, T = ops.shape[:2]
    assert keys0.shape == (S, 64) and meta.shape == (S, 4) and ops.shape == (S, T, 4) and iv.shape == (S, T, 4)
    return _launch(name, [keys0, meta, ops, iv], [((S, T, 64), "u32"), ((S, T, OI_W), "u32"), ((S, T, 4), "f64")], T, S)


def bounds(n, a1, b1, a3, b3):
    """-> (lb, ub, ctr) float64 [3][N], (klb, kub) uint32 [2][N]."""
    rows = _u32(np.stack([_u32(n), _u32(a1), _u32(b1), _u32(a3), _u32(b3)]))
    N = rows.shape[1]
    od, ou = _launch("bounds", [rows], [((3, N), "f64"), ((2, N), "u32")], N)
    return od, ou


def moments(n, n_full, lb, ub, A1, A2, T1, T2):
    """-> (mean, sd, inv_sd) float64 [3][N]; n == n_full takes the reciprocal form of the divisions."""
    ni = _i32(np.stack([_i32(n), _i32(n_full)]))
    nf = np.asarray(n_full, dtype=np.float64)
    rc = np.divide(1.0, nf, out=np.zeros_like(nf), where=nf != 0)
    d = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.float64) for x in (lb, ub, A1, A2, T1, T2, rc)]))
    N = d.shape[1]
    (o,) = _launch("moments", [ni, d], [((3, N), "f64")], N)
    return o


def refill(which, ring, win, meta):
    """which: 'refill5' | 'refill10' | 'refill_coop'; ring [n][HIST], win [n][64], meta [n][8] = r0, hi, dir, k, n, patch_slot, patch_x, side
    -> (keys [n][NW][64], (r0, hi) [n][NW][2])."""
    ring, win, meta = _u32(ring), _u32(win), _i32(meta)
    n = len(ring)
    assert ring.shape == (n, HIST) and win.shape == (n, 64) and meta.shape == (n, 8)
    nw = COOP_NW if which == "refill_coop" else 1
    return _launch(which, [ring, win, meta], [((n, nw, 64), "u32"), ((n, nw, 2), "i32")], n)


RB_I = dict(q1=0, q3=2, bu=4, bl=6, qc=8, klb=10, kub=11, ok=12)
RB_D = dict(A1=0, A2=1, qs1=2, qs2=4, mean=6, sd=7, lb=8, ub=9, ctr=10)


def rebuild(ring, meta):
    """ring [n][HIST], meta [n][4] = n, patch_slot, patch_x, 0 -> (keys [n][4][64] = q1, q3, bu, bl; oi [n][16]; od [n][12])."""
    ring, meta = _u32(ring), _i32(meta)
    n = len(ring)
    assert ring.shape == (n, HIST) and meta.shape == (n, 4)
    return _launch("rebuild", [ring, meta], [((n, 4, 64), "u32"), ((n, 16), "i32"), ((n, 12), "f64")], n)


def bisect_build(ring, meta):
    """ring [n][HIST], meta [n][8] = n, A1, B1, A3, B3, 0, 0, 0 -> (keys at the four ranks [n][4], windows [n][2][64], (r0, hi) x 2 [n][4])."""
    ring, meta = _u32(ring), _i32(meta)
    n = len(ring)
    assert ring.shape == (n, HIST) and meta.shape == (n, 8)
    return _launch("bisect_build", [ring, meta], [((n, 4), "u32"), ((n, 2, 64), "u32"), ((n, 4), "i32")], n)
