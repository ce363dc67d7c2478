"""The CPU restatement of a sample set of M members (rtggx_set_sample_set; include/rtggx.h, DESIGN.md "Sample-set size"):
tests/sampleset_ref.cpp -- the whole CPU oracle, unchanged, plus its own getSampleParam for a set of M, its own M-entry table and the path
functions of tests/recursion_ref.cpp / tests/spp_ref.cpp indexing that table -- compiled on first use with the oracle Makefile's flags into
a git-ignored library next to it, and an Oracle whose ray_trace() traces `samples` paths of `depth` levels per covered pixel and image with
samples drawn from a set of `sample_set`.  Everything else of the oracle (visibility, denoiser, tone map) is its own code, unchanged."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "sampleset_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "libsampleset_ref.so")
_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse4.1", "-fPIC"]      # oracle/Makefile CXXFLAGS

_lib = None


def build():
    deps = [_SRC] + [os.path.join(O._HERE, f) for f in os.listdir(O._HERE) if f.endswith((".h", ".cpp"))]
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
    """The library, with the oracle's ctypes signatures (copied from the oracle's own loader) and the restatement's."""
    global _lib
    if _lib is None:
        base = O.lib()
        L = C.CDLL(build())
        for name, fn in list(vars(base).items()):
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        L.orc_ray_trace_sampleset.restype = C.c_uint64
        L.orc_ray_trace_sampleset.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.orc_sample_param_m.restype = None
        L.orc_sample_param_m.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
        L.orc_sample_table_m.restype = None
        L.orc_sample_table_m.argtypes = [C.c_uint32, C.c_void_p]
        L.orc_distinct_slots_m.restype = None
        L.orc_distinct_slots_m.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        _lib = L
    return _lib


def sample_param(x, y, width, index, sample_set):
    """(s, xi.x, xi.y) of the sample with index `index` at pixel (x, y) of a frame `width` wide, from a set of `sample_set` (fp32 values)."""
    s, xi = C.c_uint32(), np.zeros(2, np.float32)
    lib().orc_sample_param_m(x, y, width, index, sample_set, C.byref(s), xi.ctypes.data_as(C.c_void_p))
    return int(s.value), xi[0], xi[1]


def sample_table(sample_set):
    """The restatement's table: float32 [sample_set, 2] of (cos, sin)(2 pi s / sample_set)."""
    t = np.zeros((sample_set, 2), np.float32)
    lib().orc_sample_table_m(sample_set, t.ctypes.data_as(C.c_void_p))
    return t


def distinct_slots(width, height, begin, end, sample_set):
    """Per pixel, the number of distinct slots the indices [begin, end) visit: uint32 [height, width]."""
    n = np.zeros((height, width), np.uint32)
    lib().orc_distinct_slots_m(width, height, begin, end, sample_set, n.ctypes.data_as(C.c_void_p))
    return n


class Oracle(O.Oracle):
    """O.Oracle on the restatement's library; ray_trace() traces `samples` (1, 2, 4, 8) paths of `depth` levels (1..4) per covered pixel,
    their samples drawn from a set of `sample_set` (a power of two, 256..65536)."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256):
        self.depth, self.samples, self.sample_set = depth, samples, sample_set
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

    def set_sample_set(self, sample_set):
        self.sample_set = int(sample_set)

    def ray_trace(self):
        return int(self.L.orc_ray_trace_sampleset(self.h, C.c_uint32(self.depth), C.c_uint32(self.samples), C.c_uint32(self.sample_set)))
