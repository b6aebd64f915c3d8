"""The one copy of what the function-level probes (tests/physics_probe.py, tests/reward_probe.py) share: build tests/aux/<name>.hip
with the library's own flags (dc_rl_amd._lib.HIPCC_FLAGS) into tests/aux/build/lib<name>.so when it is stale, and load it.

TEST INFRASTRUCTURE ONLY.  __graft_entry__.build() builds every probe beside the oracle; the GPU machine runs what build() made, so a
missing library is an error that names the build command, never a build on import.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from dc_rl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT_DIR = os.path.join(HERE, "aux", "build")          # (git-ignored: build/)


class Probe:
    def __init__(self, name: str, what: str):
        self.name, self.what = name, what
        self.src = os.path.join(HERE, "aux", name + ".hip")
        self.lib_path = os.path.join(OUT_DIR, "lib" + name + ".so")
        self.build_hint = ("python -c 'import __graft_entry__ as g; g.build()'   "
                           f"(or: python -c 'from tests import {name} as p; p.build()')")
        self._lib = None

    def build_command(self, out_path=None, flags=None):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        flags = list(L.HIPCC_FLAGS if flags is None else flags)
        return [hipcc] + flags + ["-I", L.CSRC, self.src, "-o", out_path or self.lib_path]

    def deps(self):
        return [self.src, os.path.abspath(L.__file__), os.path.join(ROOT, "include", "sustaindc_hip.h")] + \
               [os.path.join(L.CSRC, f) for f in os.listdir(L.CSRC) if f.endswith(".hpp")]

    def build(self, force: bool = False, verbose: bool = False) -> str:
        """hipcc (cross-compiles gfx950 without a GPU) -> tests/aux/build/lib<name>.so; a few seconds."""
        lib = self.lib_path
        if not force and os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(d) for d in self.deps()):
            return lib
        os.makedirs(OUT_DIR, exist_ok=True)
        tmp = lib + f".{os.getpid()}.tmp"                  # (several test workers may build at once: the rename is atomic)
        cmd = self.build_command(tmp)
        if verbose:
            print(" ".join(cmd))
        try:
            subprocess.check_call(cmd, cwd=ROOT)
            os.replace(tmp, lib)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        return lib

    def load(self, declare):
        """The loaded probe; declare(lib) sets the launchers' argument types once.  A missing probe is an error that names the build
        command."""
        if self._lib is None:
            import torch  # noqa: F401  (maps PyTorch-ROCm's HIP runtime first, as dc_rl_amd._lib.load does)
            if not os.path.exists(self.lib_path):
                raise RuntimeError(f"the {self.what} is not built: {self.lib_path} is missing.  Run {self.build_hint}")
            lib = C.CDLL(self.lib_path)
            declare(lib)
            self._lib = lib
        return self._lib
