"""The CPU restatements of the settings the reference does not have, in one library: tests/restatements.cpp -- the whole CPU oracle
(oracle/orc_capi.cpp) once, plus orc_ray_trace_depth (tests/recursion_ref.cpp: recursion depth D, rtggx_set_max_recursion_depth),
orc_ray_trace_spp (tests/spp_ref.cpp: N samples per pixel, rtggx_set_samples_per_pixel) and orc_ray_trace_sampleset
(tests/sampleset_ref.cpp: a sample set of M members, rtggx_set_sample_set) -- compiled on first use into a git-ignored library, and an
Oracle whose ray_trace() is one of the three.  Everything else of the oracle (visibility, denoiser, tone map) is its own code, unchanged.
Each layer reproduces the one below it bit for bit at its default: depth 1 the oracle (tests/test_recursion_host.py), one sample the depth
restatement (tests/test_spp_host.py), M = 256 the spp restatement (tests/test_sampleset_host.py)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "restatements.cpp")
_OUT = os.path.join(_HERE, "_build", "librestatement.so")
_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse4.1", "-fPIC"]      # oracle/Makefile CXXFLAGS, less its warnings

_lib = None


def build():
    deps = [os.path.join(d, f) for d, ends in ((_HERE, (".cpp",)), (O._HERE, (".h", ".cpp"))) for f in os.listdir(d) if f.endswith(ends)]
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
        L = C.CDLL(build())
        for name, fn in list(vars(O.lib()).items()):
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        u32 = C.c_uint32
        for name, restype, argtypes in (
                ("orc_ray_trace_depth", C.c_uint64, [C.c_void_p, u32]),
                ("orc_ray_trace_spp", C.c_uint64, [C.c_void_p, u32, u32]),
                ("orc_ray_trace_spp_f32", C.c_uint64, [C.c_void_p, u32, u32, C.c_void_p, C.c_void_p]),
                ("orc_ray_trace_spp_primary_f32", C.c_uint64, [C.c_void_p, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p]),
                ("orc_ray_trace_sampleset", C.c_uint64, [C.c_void_p, u32, u32, u32]),
                ("orc_sample_param_m", None, [u32, u32, u32, u32, u32, C.POINTER(u32), C.c_void_p]),
                ("orc_sample_table_m", None, [u32, C.c_void_p]),
                ("orc_distinct_slots_m", None, [u32, u32, u32, u32, u32, C.c_void_p])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def sample_param(x, y, width, index, sample_set):
    """(s, xi.x, xi.y) of the sample with index `index` at pixel (x, y) of a frame `width` wide, from a set of `sample_set` (fp32 values)."""
    s, xi = C.c_uint32(), np.zeros(2, np.float32)
    lib().orc_sample_param_m(x, y, width, index, sample_set, C.byref(s), xi.ctypes.data_as(C.c_void_p))
    return int(s.value), xi[0], xi[1]


def sample_table(sample_set):
    """The sample-set restatement's table: float32 [sample_set, 2] of (cos, sin)(2 pi s / sample_set)."""
    t = np.zeros((sample_set, 2), np.float32)
    lib().orc_sample_table_m(sample_set, t.ctypes.data_as(C.c_void_p))
    return t


def distinct_slots(width, height, begin, end, sample_set):
    """Per pixel, the number of distinct slots the indices [begin, end) visit: uint32 [height, width]."""
    n = np.zeros((height, width), np.uint32)
    lib().orc_distinct_slots_m(width, height, begin, end, sample_set, n.ctypes.data_as(C.c_void_p))
    return n


ENTRIES = {"depth": ("orc_ray_trace_depth", 1), "spp": ("orc_ray_trace_spp", 2), "sampleset": ("orc_ray_trace_sampleset", 3)}      # (C function, how many of depth, samples, sample_set it takes)


class Oracle(O.Oracle):
    """O.Oracle on the restatements' library.  ray_trace() traces `samples` (1, 2, 4, 8) paths of `depth` levels (1..4) per covered pixel and
    image, their samples drawn from a set of `sample_set` (a power of two, 256..65536), through the C function `entry` names: "depth"
    (orc_ray_trace_depth: one sample, the set of 256), "spp" (orc_ray_trace_spp: the set of 256) or "sampleset" (orc_ray_trace_sampleset).
    A setting its entry point does not take is held and not used."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256, entry="sampleset"):
        self.depth, self.samples, self.sample_set = depth, samples, sample_set
        self.entry, self.taken = ENTRIES[entry]
        super().__init__(width, height, threads, lib=lib())

    def set_max_recursion_depth(self, depth):
        self.depth = int(depth)

    def set_samples_per_pixel(self, samples):
        self.samples = int(samples)

    def set_sample_set(self, sample_set):
        self.sample_set = int(sample_set)

    def ray_trace_function(self):
        """(the C function ray_trace() calls, its arguments after the handle)"""
        return getattr(self.L, self.entry), [C.c_uint32(v) for v in (self.depth, self.samples, self.sample_set)[:self.taken]]

    def ray_trace(self):
        fn, args = self.ray_trace_function()
        return int(fn(self.h, *args))

    def ray_trace_f32(self, samples=None):
        """orc_ray_trace_spp with `samples` (any count; default: the setting) that also returns the two images before packing, fp32 [H, W, 3];
        a pixel without a diffuse path keeps NaN in the second."""
        n = self.samples if samples is None else int(samples)
        refl = np.full((self.H, self.W, 3), np.nan, np.float32)
        diff = np.full((self.H, self.W, 3), np.nan, np.float32)
        rays = int(self.L.orc_ray_trace_spp_f32(self.h, C.c_uint32(self.depth), C.c_uint32(n), refl.ctypes.data_as(C.c_void_p), diff.ctypes.data_as(C.c_void_p)))
        return rays, refl, diff

    def ray_trace_primary_f32(self):
        """ray_trace_f32 at the setting, and the primary surface in front of the G-buffer's packs: fp32 [H, W, 6] of N * 0.5 + 0.5, the velocity
        and the roughness."""
        refl = np.full((self.H, self.W, 3), np.nan, np.float32)
        diff = np.full((self.H, self.W, 3), np.nan, np.float32)
        primary = np.zeros((self.H, self.W, 6), np.float32)
        rays = int(self.L.orc_ray_trace_spp_primary_f32(self.h, C.c_uint32(self.depth), C.c_uint32(self.samples), refl.ctypes.data_as(C.c_void_p),
                                                        diff.ctypes.data_as(C.c_void_p), primary.ctypes.data_as(C.c_void_p)))
        return rays, refl, diff, primary

    def ray_trace_depth_restatement(self):
        """tests/recursion_ref.cpp's orc_ray_trace_depth, for comparison with the spp entry at one sample."""
        return int(self.L.orc_ray_trace_depth(self.h, C.c_uint32(self.depth)))

    def ray_trace_oracle(self):
        """The oracle's own orc_ray_trace (raygen_pixel), for comparison with the restatements at one sample and depth 1."""
        return int(self.L.orc_ray_trace(self.h))

    ray_trace_depth1_oracle = ray_trace_oracle      # (the name of the recursion tests)
