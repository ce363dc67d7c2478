"""The CPU restatement of the sun at the surfaces the paths hit (rtggx_set_sun_reflections): tests/sun_hit_ref.cpp -- tests/sun_ref.cpp, i.e.
the whole oracle, every restatement and orc_sun_apply, plus orc_ray_trace_sun_hits -- compiled on first use like sun_ref.py's library; an
Oracle with set_sun_reflections whose ray_trace() walks the paths through that function (with the toggle off, or without a sun, it is
sampleset_ref.cpp's walker once more) and applies the primary pass behind it; and mapped_frame() for frames under a sample map."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import adaptive_ref as AD
import restatement as RS
import sun_ref as SR
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "sun_hit_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "libsun_hit_ref.so")
COLUMNS = ("miss", "preset", "facing_away", "occluded", "lit", "specular", "diffuse")      # per level; the two lobes among the sun-facing hits
CLASSES = ("facing_away", "occluded", "lit")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [os.path.join(d, f) for d, ends in ((_HERE, (".cpp",)), (O._HERE, (".h", ".cpp"))) for f in os.listdir(d) if f.endswith(ends)]
        if not (os.path.exists(_OUT) and all(os.path.getmtime(d) <= os.path.getmtime(_OUT) for d in deps)):
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            fd, tmp = tempfile.mkstemp(suffix=".so", dir=os.path.dirname(_OUT))
            os.close(fd)
            try:
                subprocess.check_call([os.environ.get("CXX", "g++")] + RS._FLAGS + ["-shared", "-pthread", "-o", tmp, _SRC])
                os.replace(tmp, _OUT)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
        L = C.CDLL(_OUT)
        for name, fn in list(vars(SR.lib()).items()):      # the signatures of the oracle's, the restatements' and the sun's functions
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        u32 = C.c_uint32
        L.orc_sun_hit_columns.restype, L.orc_sun_hit_columns.argtypes = u32, []
        L.orc_ray_trace_sun_hits.restype = C.c_uint64
        L.orc_ray_trace_sun_hits.argtypes = [C.c_void_p, u32, u32, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p]
        assert L.orc_sun_hit_columns() == len(COLUMNS)
        _lib = L
    return _lib


class Oracle(SR.Oracle):
    """SR.Oracle whose paths are walked by orc_ray_trace_sun_hits.  counts: uint64 [4, len(COLUMNS)] of the last frame, by level; lit: uint8
    [H, W], bit 0 / 1 where a term exists in RayTracingOut0 / 1; hit_rays: the shadow rays from hits of the last frame."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256):
        self.depth, self.samples, self.sample_set = depth, samples, sample_set
        self.entry, self.taken = RS.ENTRIES["sampleset"]
        self.sun, self.sun_reflections = None, False
        self.force_sums = self.keep_counts = False
        self.classes = np.zeros((height, width), np.uint8)
        self.lit = np.zeros((height, width), np.uint8)
        self.counts = np.zeros((4, len(COLUMNS)), np.uint64)
        O.Oracle.__init__(self, width, height, threads, lib=lib())

    def set_sun_reflections(self, on):
        self.sun_reflections = bool(on)

    def count(self, name, level=None):
        col = self.counts[:, COLUMNS.index(name)]
        return int(col.sum() if level is None else col[level])

    @property
    def hit_rays(self):
        return self.count("occluded") + self.count("lit")

    def ray_trace(self):
        on = self.sun is not None and self.sun_reflections
        l, e = self.sun if self.sun is not None else (np.zeros(3, np.float32), np.zeros(3, np.float32))
        if not self.keep_counts:
            self.counts[...] = 0
        lit = np.zeros_like(self.lit)
        rays = int(self.L.orc_ray_trace_sun_hits(self.h, self.depth, self.samples, self.sample_set, l.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                                                 (1 if on else 0) | (2 if self.force_sums else 0), self.counts.ctypes.data_as(C.c_void_p), lit.ctypes.data_as(C.c_void_p)))
        self.lit = lit | self.lit if self.keep_counts else lit
        return rays + (self.sun_apply() if self.sun is not None else 0)


def mapped_frame(o, blocks):
    """adaptive_ref.mapped_frame for an Oracle of this module: every block's terms go into its fp32 sums, whatever its count -- the frame is
    an N-sample frame -- and the counts and the lit map are those of the composed frame.  (classes: of the last part only.)"""
    o.counts[...] = 0
    o.lit[...] = 0
    o.force_sums = o.keep_counts = True
    try:
        return AD.mapped_frame(o, blocks)
    finally:
        o.force_sums = o.keep_counts = False
