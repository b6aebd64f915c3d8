"""Build and drive tests/aux/physics_probe.hip: the step's shared arithmetic (dc_rl_amd/csrc/sdc_physics.hpp), one function per
kernel and one element per thread, with the constants from either of the two sources the step kernels use.

TEST INFRASTRUCTURE ONLY.  The probe is compiled with the library's own flags (dc_rl_amd._lib.HIPCC_FLAGS: -ffp-contract=off and the
scheduling options included), so it holds the bits the library ships; __graft_entry__.build() builds it beside the oracle.
"""
from __future__ import annotations

import ctypes as C

from tests.probe_build import OUT_DIR, ROOT, Probe                                 # (the build / staleness / load logic both probes share)

# launcher -> (input rows, output rows); tests/aux/physics_probe.hip lists what each row is
KERNELS = {
    "log2_pos_normal": (1, 1), "exp2_plain": (1, 1), "exp_plain": (1, 1), "exp2_short": (1, 1), "rise": (2, 1),
    "div_const": (3, 1), "div_fast": (2, 1), "chiller_power": (3, 1), "rack_point": (16, 5), "rack_wide": (16, 5),
    "hvac_water": (11, 4), "battery_step": (6, 6),
}
KLIT, KLDS = 0, 1
SOURCES = (("KLit", KLIT), ("KLds", KLDS))

_PROBE = Probe("physics_probe", "physics probe")
SRC, LIB_PATH, BUILD_HINT = _PROBE.src, _PROBE.lib_path, _PROBE.build_hint
build_command, build = _PROBE.build_command, _PROBE.build


def _declare(lib):
    for name in KERNELS:
        fn = getattr(lib, "probe_" + name)
        fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        fn.restype = C.c_int


def load():
    """The loaded probe.  A missing probe is an error that names the build command: the GPU machine runs what build() made."""
    return _PROBE.load(_declare)


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
