"""Build and drive tests/aux/physics_probe.hip: the step's shared arithmetic (dc_rl_amd/csrc/sdc_physics.hpp), one function per
kernel and one element per thread, with the constants from either of the two sources the step kernels use.

TEST INFRASTRUCTURE ONLY.  The probe is compiled with the library's own flags (dc_rl_amd._lib.HIPCC_FLAGS: -ffp-contract=off and the
scheduling options included), so it holds the bits the library ships; __graft_entry__.build() builds it beside the oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from dc_rl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "aux", "physics_probe.hip")
OUT_DIR = os.path.join(HERE, "aux", "build")          # (git-ignored: build/)
LIB_PATH = os.path.join(OUT_DIR, "libphysics_probe.so")
BUILD_HINT = "python -c 'import __graft_entry__ as g; g.build()'   (or: python -c 'from tests import physics_probe as p; p.build()')"

# launcher -> (input rows, output rows); tests/aux/physics_probe.hip lists what each row is
KERNELS = {
    "log2_pos_normal": (1, 1), "exp2_plain": (1, 1), "exp_plain": (1, 1), "exp2_short": (1, 1), "rise": (2, 1),
    "div_const": (3, 1), "div_fast": (2, 1), "chiller_power": (3, 1), "rack_point": (16, 5), "rack_wide": (16, 5),
    "hvac_water": (11, 4), "battery_step": (6, 6),
}
KLIT, KLDS = 0, 1
SOURCES = (("KLit", KLIT), ("KLds", KLDS))


def build_command(out_path: str = LIB_PATH, flags=None):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = list(L.HIPCC_FLAGS if flags is None else flags)
    return [hipcc] + flags + ["-I", L.CSRC, SRC, "-o", out_path]


def _deps():
    return [SRC, os.path.abspath(L.__file__), os.path.join(ROOT, "include", "sustaindc_hip.h")] + \
           [os.path.join(L.CSRC, f) for f in os.listdir(L.CSRC) if f.endswith(".hpp")]


def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc (cross-compiles gfx950 without a GPU) -> tests/aux/build/libphysics_probe.so; a few seconds."""
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(d) for d in _deps()):
        return LIB_PATH
    os.makedirs(OUT_DIR, exist_ok=True)
    tmp = LIB_PATH + f".{os.getpid()}.tmp"             # (several test workers may build at once: the rename is atomic)
    cmd = build_command(tmp)
    if verbose:
        print(" ".join(cmd))
    try:
        subprocess.check_call(cmd, cwd=ROOT)
        os.replace(tmp, LIB_PATH)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return LIB_PATH


_lib = None


def load():
    """The loaded probe.  A missing probe is an error that names the build command: the GPU machine runs what build() made."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (maps PyTorch-ROCm's HIP runtime first, as dc_rl_amd._lib.load does)
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"the physics probe is not built: {LIB_PATH} is missing.  Run {BUILD_HINT}")
        lib = C.CDLL(LIB_PATH)
        for name in KERNELS:
            fn = getattr(lib, "probe_" + name)
            fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
            fn.restype = C.c_int
        _lib = lib
    return _lib


def run(name: str, source: int, *rows):
    """Launch probe_<name> on the current stream of cuda:0.  rows: one array per input row (NumPy or anything np.asarray takes,
    scalars are broadcast); returns the output rows as a float64 NumPy array [n_out, n]."""
    import numpy as np
    import torch
    n_in, n_out = KERNELS[name]
    assert len(rows) == n_in, (name, len(rows), n_in)
    host = np.ascontiguousarray(np.stack(np.broadcast_arrays(*[np.asarray(r, dtype=np.float64) for r in rows])))
    assert host.ndim == 2, "inputs are one-dimensional"
    n = host.shape[1]
    dev = torch.device("cuda", 0)
    din = torch.from_numpy(host).to(dev)
    dout = torch.full((n_out, n), float("nan"), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(load(), "probe_" + name)(int(source), din.data_ptr(), dout.data_ptr(), n,
                                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"probe_{name}: hipError {rc}"
        torch.cuda.synchronize()
    return dout.cpu().numpy()


def run_both(name: str, *rows):
    """Both constant sources; asserts KLit == KLds bit for bit on every output row and returns one of them."""
    import numpy as np
    lit = run(name, KLIT, *rows)
    lds = run(name, KLDS, *rows)
    same = lit.view(np.uint64) == lds.view(np.uint64)
    assert same.all(), (f"{name}: the literal and the LDS-table constants give different bits at {int((~same).sum())} of {same.size} "
                        f"outputs, first at (row, element) {tuple(np.argwhere(~same)[0])}")
    return lit
