"""ctypes binding of tests/native/ggx_twin.cpp — the oracle with the reference's closure switch (`#define BRDF`, Renderer.hpp:70)
made a runtime argument and the gloss decay table supplied by the caller.  TEST INFRASTRUCTURE ONLY.

The twin is compiled on first use with oracle/Makefile's CXXFLAGS into a temporary directory (never into the repository, never
linked into the product).  It includes oracle/oracle.cpp whole, so it exports every orc_* entry point too: `GgxTwin` is the
oracle_binding.Oracle call protocol on that library, with `Accumulate` going through the closure switch."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import oracle_binding as ob

ROOT = ob.ROOT
SRC = os.path.join(ROOT, "tests", "native", "ggx_twin.cpp")
_lib = None


def oracle_cxxflags():
    """CXXFLAGS exactly as oracle/Makefile sets them."""
    text = open(os.path.join(ob.ORACLE_DIR, "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", text, flags=re.M)
    return m.group(1).split()


def build(out_dir=None):
    out_dir = out_dir or tempfile.mkdtemp(prefix="ggx_twin_")
    so = os.path.join(out_dir, "libggx_twin.so")
    subprocess.run(["g++", *oracle_cxxflags(), "-shared", "-o", so, SRC], check=True)
    return so


def load(so=None):
    """dlopen the twin (building it when `so` is not given) with the oracle's argument types on every orc_* symbol."""
    global _lib
    if _lib is not None:
        return _lib
    so = so or build()
    lib = C.CDLL(so)
    ref = ob.load()
    for name in dir(ref):
        if name.startswith("orc_"):
            src, dst = getattr(ref, name), getattr(lib, name)
            if getattr(src, "argtypes", None) is not None:
                dst.argtypes = src.argtypes
            dst.restype = src.restype
    lib.ggx_twin_accumulate.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32]
    lib.ggx_twin_accumulate.restype = C.c_int
    _lib = lib
    return lib


class GgxTwin(ob.Oracle):
    """oracle_binding.Oracle with `brdf` (0 Lambertian, 1 GGX) and a gloss decay table."""

    def __init__(self, scene, brdf=0, gloss_decay=None, **kw):
        self.brdf = int(brdf)
        self.set_gloss_decay(gloss_decay)
        lib = load()
        saved, ob._lib = ob._lib, lib          # Oracle.__init__ takes its library from oracle_binding.load()
        try:
            super().__init__(scene, **kw)
        finally:
            ob._lib = saved

    def set_gloss_decay(self, decay=None):
        self.decay = np.ascontiguousarray([] if decay is None else decay, dtype=np.float32).reshape(-1)

    def Accumulate(self, n_calls=1):
        d = self.decay
        rc = self.lib.ggx_twin_accumulate(self.h, n_calls, self.brdf, d.ctypes.data_as(C.c_void_p) if len(d) else None, len(d))
        assert rc == 0
