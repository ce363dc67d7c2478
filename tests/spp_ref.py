"""The CPU restatement of N samples per pixel (rtggx_set_samples_per_pixel; include/rtggx.h, DESIGN.md "Samples per pixel"): tests/spp_ref.cpp
-- tests/recursion_ref.cpp, i.e. the whole CPU oracle and the path loop, plus orc_ray_trace_spp -- compiled on first use with the oracle
Makefile's flags into a git-ignored library next to it, and an Oracle whose ray_trace() traces `samples` paths of `depth` levels per covered
pixel and image.  Everything else of the oracle (visibility, denoiser, tone map) is its own code, unchanged."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "spp_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "libspp_ref.so")
_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse4.1", "-fPIC"]      # oracle/Makefile CXXFLAGS

_lib = None


def build():
    deps = [_SRC, os.path.join(_HERE, "recursion_ref.cpp")] + [os.path.join(O._HERE, f) for f in os.listdir(O._HERE) if f.endswith((".h", ".cpp"))]
    if os.path.exists(_OUT) and all(os.path.getmtime(d) <= os.path.getmtime(_OUT) for d in deps):
        return _OUT
    os.makedirs(os.path.dirname(_OUT), exist_ok=True)
    fd, tmp = tempfile.mkstemp(suffix=".so", dir=os.path.dirname(_OUT))
    os.close(fd)
    try:
        subprocess.check_call([os.environ.get("CXX", "g++")] + _FLAGS + ["-shared", "-pthread", "-o", tmp, _SRC])
        os.replace(tmp, _OUT)      # (atomic: a concurrent first use sees the old library or the new one)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return _OUT


def lib():
    """The library, with the oracle's ctypes signatures (copied from the oracle's own loader) and the restatements'."""
    global _lib
    if _lib is None:
        base = O.lib()
        L = C.CDLL(build())
        for name, fn in list(vars(base).items()):
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        L.orc_ray_trace_depth.restype = C.c_uint64
        L.orc_ray_trace_depth.argtypes = [C.c_void_p, C.c_uint32]
        L.orc_ray_trace_spp.restype = C.c_uint64
        L.orc_ray_trace_spp.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.orc_ray_trace_spp_f32.restype = C.c_uint64
        L.orc_ray_trace_spp_f32.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


class Oracle(O.Oracle):
    """O.Oracle on the restatement's library; ray_trace() traces `samples` (1, 2, 4, 8) paths of `depth` levels (1..4) per covered pixel."""

    def __init__(self, width, height, threads=None, depth=1, samples=1):
        self.depth, self.samples = depth, samples
        L, O_lib = lib(), O._lib
        O._lib = L      # (O.Oracle.__init__ takes its library from O.lib())
        try:
            super().__init__(width, height, threads)
        finally:
            O._lib = O_lib

    def set_max_recursion_depth(self, depth):
        self.depth = int(depth)

    def set_samples_per_pixel(self, samples):
        self.samples = int(samples)

    def ray_trace(self):
        return int(self.L.orc_ray_trace_spp(self.h, C.c_uint32(self.depth), C.c_uint32(self.samples)))

    def ray_trace_f32(self, samples=None):
        """ray_trace() with `samples` (any count; default: the setting) that also returns the two images before packing, fp32 [H, W, 3];
        a pixel without a diffuse path keeps NaN in the second."""
        n = self.samples if samples is None else int(samples)
        refl = np.full((self.H, self.W, 3), np.nan, np.float32)
        diff = np.full((self.H, self.W, 3), np.nan, np.float32)
        rays = int(self.L.orc_ray_trace_spp_f32(self.h, C.c_uint32(self.depth), C.c_uint32(n), refl.ctypes.data_as(C.c_void_p), diff.ctypes.data_as(C.c_void_p)))
        return rays, refl, diff

    def ray_trace_depth_restatement(self):
        """tests/recursion_ref.cpp's orc_ray_trace_depth, for comparison with ray_trace() at one sample."""
        return int(self.L.orc_ray_trace_depth(self.h, C.c_uint32(self.depth)))

    def ray_trace_oracle(self):
        """The oracle's own orc_ray_trace (raygen_pixel), for comparison with ray_trace() at one sample and depth 1."""
        return int(self.L.orc_ray_trace(self.h))
