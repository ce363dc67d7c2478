"""The CPU restatement of a sun with a size (rtggx_set_sun_angle): tests/sun_soft_ref.cpp -- tests/sun_hit_ref.cpp, i.e. the whole oracle,
every restatement, orc_sun_apply and orc_ray_trace_sun_hits, plus the rule's direction, the primary pass and the path walker with it --
compiled on first use like sun_hit_ref.py's library; the host's k, T and B (disk), following sun_ref.normalise; an Oracle with
set_sun_angle whose ray_trace() goes through the new functions while the angle is above 0 and through sun_hit_ref's otherwise; and
mapped_frame() for frames under a sample map."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

import adaptive_ref as AD
import restatement as RS
import sun_hit_ref as SH
import sun_ref as SR
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "sun_soft_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "libsun_soft_ref.so")
MAX_ANGLE = 10.0
NOT_COVERED, FACING_AWAY, OCCLUDED, LIT, BELOW_HORIZON = 0, 1, 2, 3, 4
SOFT_COLUMNS = ("below_horizon", "differs")      # per level: hits below the horizon; hits whose sampled ray's outcome differs from the centre ray's
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
        for name, fn in list(vars(SH.lib()).items()):      # the signatures of the oracle's, the restatements' and the sun's functions
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        u32, vp, f32 = C.c_uint32, C.c_void_p, C.c_float
        L.orc_sun_disk_sample.restype, L.orc_sun_disk_sample.argtypes = None, [u32, u32, u32, vp, vp, vp, f32, vp]
        L.orc_sun_soft_apply.restype, L.orc_sun_soft_apply.argtypes = C.c_uint64, [vp, vp, vp, vp, vp, f32, u32, vp, vp, u32]
        L.orc_ray_trace_sun_soft_hits.restype = C.c_uint64
        L.orc_ray_trace_sun_soft_hits.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, f32, u32, vp, vp, vp, vp]
        _lib = L
    return _lib


def disk(l, degrees):
    """The host's rule (include/rtggx.h): (k, T, B) in double on the fp32 direction `l` (sun_ref.normalise's), each rounded once to fp32."""
    l = np.asarray(l, np.float32).astype(np.float64)
    k = np.float32(1.0 - math.cos(float(np.float32(degrees)) * 3.14159265358979323846 / 180.0))
    a = int(np.argmin(np.abs(l)))      # (the first of equal ones)
    t = np.zeros(3)
    t[(a + 1) % 3], t[(a + 2) % 3] = -l[(a + 2) % 3], l[(a + 1) % 3]      # cross(e_a, L)
    t = t / math.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
    b = np.array([l[1] * t[2] - l[2] * t[1], l[2] * t[0] - l[0] * t[2], l[0] * t[1] - l[1] * t[0]])
    return k, t.astype(np.float32), b.astype(np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def sample(pixel, frame_index, j, l, degrees):
    """(Ls as three fp32, u, s) of the rule's steps 1-5."""
    k, t, b = disk(l, degrees)
    out = np.zeros(5, np.float32)
    lib().orc_sun_disk_sample(pixel, frame_index, j, _p(np.ascontiguousarray(l, np.float32)), _p(t), _p(b), k, _p(out))
    return out[:3].copy(), float(out[3]), int(out[4])


class Oracle(SH.Oracle):
    """SH.Oracle with the angle.  classes: the class map of the last primary pass by the sampled ray, 4 below the horizon; centre: the
    directional sun's classes of the same pixels (statistics on); soft: uint64 [4, len(SOFT_COLUMNS)] by level; changed: uint8 [H, W], bit
    0 / 1 where a hit of the path writing RayTracingOut0 / 1 is below the horizon or (statistics on) differs from the centre ray's outcome.
    primary_index: the frame index the primary pass draws with when it is not the constants' (a part of a mapped frame).  force_rule: the
    new functions are used at angle 0 as well -- k = 0, where the rule gives e = 0, sin(theta) = 0 and Ls = L exactly -- instead of
    sun_hit_ref's: what shows that the copied walker and primary pass have not drifted from theirs."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256):
        self.depth, self.samples, self.sample_set = depth, samples, sample_set      # (SH.Oracle's, on this module's library)
        self.entry, self.taken = RS.ENTRIES["sampleset"]
        self.sun, self.sun_reflections = None, False
        self.force_sums = self.keep_counts = False
        self.classes = np.zeros((height, width), np.uint8)
        self.lit = np.zeros((height, width), np.uint8)
        self.counts = np.zeros((4, len(SH.COLUMNS)), np.uint64)
        self.angle, self.statistics, self.primary_index, self.force_rule = 0.0, False, None, False
        self.centre = np.zeros((height, width), np.uint8)
        self.changed = np.zeros((height, width), np.uint8)
        self.soft = np.zeros((4, len(SOFT_COLUMNS)), np.uint64)
        O.Oracle.__init__(self, width, height, threads, lib=lib())

    def set_sun_angle(self, degrees):
        """Refuses what the product refuses, keeping the angle."""
        d = float(np.float32(degrees))
        if not (0.0 <= d <= MAX_ANGLE):
            raise ValueError("angle %r" % (degrees,))
        self.angle = d

    def soft_count(self, name, level=None):
        col = self.soft[:, SOFT_COLUMNS.index(name)]
        return int(col.sum() if level is None else col[level])

    def _frame_index(self):
        return int(self.get_frame_constants()[444:448].view(np.uint32)[0])

    def sun_apply(self):
        if not (self.angle > 0.0 or self.force_rule):
            return SH.Oracle.sun_apply(self)
        l, e = self.sun
        k, t, b = disk(l, self.angle)
        index = self._frame_index() if self.primary_index is None else self.primary_index
        classes, centre = np.zeros_like(self.classes), np.zeros_like(self.centre)
        rays = int(self.L.orc_sun_soft_apply(self.h, _p(l), _p(e), _p(t), _p(b), k, index, _p(classes), _p(centre) if self.statistics else None, 0))
        if self.keep_counts:      # a part of a mapped frame: its pixels are the covered ones
            classes, centre = np.where(classes != 0, classes, self.classes), np.where(classes != 0, centre, self.centre)
        self.classes[...], self.centre[...] = classes, centre
        return rays

    def lit_words(self):
        """(RayTracingOut0, RayTracingOut1) as the directional sun leaves them where nothing occludes it, from the oracle's words as they
        are (a frame traced without a sun); the oracle's words are put back."""
        l, e = self.sun
        _, t, b = disk(l, 0.0)
        before = self.buffer(O.BUF_RT_REFL), self.buffer(O.BUF_RT_DIFF)
        self.L.orc_sun_soft_apply(self.h, _p(l), _p(e), _p(t), _p(b), np.float32(0.0), 0, None, None, 1)
        lit = self.buffer(O.BUF_RT_REFL), self.buffer(O.BUF_RT_DIFF)
        self.buffer(O.BUF_RT_REFL, copy=False)[...], self.buffer(O.BUF_RT_DIFF, copy=False)[...] = before
        return lit

    def ray_trace(self):
        on = self.sun is not None and self.sun_reflections
        if not (on and (self.angle > 0.0 or self.force_rule)):
            return SH.Oracle.ray_trace(self)      # (its primary pass is this class's sun_apply)
        l, e = self.sun
        k, t, b = disk(l, self.angle)
        if not self.keep_counts:
            self.counts[...] = 0
            self.soft[...] = 0
        lit, changed = np.zeros_like(self.lit), np.zeros_like(self.changed)
        flags = 1 | (2 if self.force_sums else 0) | (4 if self.statistics else 0)
        rays = int(self.L.orc_ray_trace_sun_soft_hits(self.h, self.depth, self.samples, self.sample_set, _p(l), _p(e), _p(t), _p(b), k, flags,
                                                      _p(self.counts), _p(lit), _p(self.soft), _p(changed)))
        self.lit = lit | self.lit if self.keep_counts else lit
        self.changed = changed | self.changed if self.keep_counts else changed
        return rays + self.sun_apply()


def mapped_frame(o, blocks):
    """sun_hit_ref.mapped_frame for an Oracle of this module: the parts' primary passes draw with the frame's own index."""
    o.soft[...] = 0
    o.changed[...] = 0
    o.classes[...] = 0
    o.centre[...] = 0
    o.primary_index = o._frame_index()
    try:
        return SH.mapped_frame(o, blocks)
    finally:
        o.primary_index = None
