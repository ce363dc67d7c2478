"""The CPU restatement of the local lights (rtggx_set_lights): tests/lights_ref.cpp -- tests/sun_soft_ref.cpp, i.e. the whole oracle, every
restatement and the three sun passes, plus the lights' pass -- compiled on first use like sun_soft_ref.py's library; the host's records
(record: the axis normalised in double and rounded once, as rtggx_set_lights does); and an Oracle with set_lights that refuses what the
product refuses and whose ray_trace() runs the lights' pass behind sun_soft_ref's frame."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

import restatement as RS
import sun_soft_ref as SS
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "lights_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "liblights_ref.so")
MAX_LIGHTS = 8
NOT_COVERED, OUT_OF_RANGE, FACING_AWAY, OUTSIDE_CONE, BELOW_HORIZON, OCCLUDED, LIT = range(7)
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
        for name, fn in list(vars(SS.lib()).items()):      # the signatures of everything below this library
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        u32, vp = C.c_uint32, C.c_void_p
        L.orc_lights_apply.restype, L.orc_lights_apply.argtypes = C.c_uint64, [vp, vp, u32, u32, vp, u32]
        L.orc_lights_apply_aux.restype, L.orc_lights_apply_aux.argtypes = C.c_uint64, [vp, vp, u32, u32, vp, u32, vp]
        L.orc_light_sphere_point.restype, L.orc_light_sphere_point.argtypes = None, [u32, u32, vp]
        L.orc_light_sphere_points.restype, L.orc_light_sphere_points.argtypes = None, [vp]
        L.orc_light_sphere_sample.restype, L.orc_light_sphere_sample.argtypes = None, [u32, u32, u32, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cone(outer_degrees, inner_degrees):
    """(cos_outer, cos_inner) as the command line makes them: cos(deg pi / 180) in double, rounded once."""
    return tuple(float(np.float32(math.cos(float(np.float32(d)) * 3.14159265358979323846 / 180.0))) for d in (outer_degrees, inner_degrees))


def record(position, intensity, range, radius=0.0, axis=(0.0, 0.0, 0.0), cos_outer=-1.0, cos_inner=1.0):
    """One light as 16 fp32 in RtggxLight's layout, checked and with the axis normalised as rtggx_set_lights does; ValueError where the
    product refuses."""
    f = np.zeros(16, np.float32)
    f[0:3], f[3], f[4:7], f[7], f[8:11], f[11], f[12] = position, range, intensity, radius, axis, cos_outer, cos_inner
    if not np.isfinite(f[0:3]).all():
        raise ValueError("position")
    if not (np.isfinite(f[3]) and f[3] > 0):
        raise ValueError("range")
    if not (np.isfinite(f[4:7]).all() and (f[4:7] >= 0).all()):
        raise ValueError("intensity")
    if not (np.isfinite(f[7]) and f[7] >= 0 and f[7] < f[3]):
        raise ValueError("radius")
    if f[11] > -1:
        a = f[8:11].astype(np.float64)
        n = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        if not (math.isfinite(n) and n > 0):
            raise ValueError("axis")
        if not (f[11] < f[12] <= 1):
            raise ValueError("cosines")
        f[8:11] = (a / n).astype(np.float32)
    elif not f[11] <= -1:
        raise ValueError("cos_outer")
    return f


def records(lights):
    """[count, 16] fp32 of a sequence of dicts (record's arguments); ValueError on more than MAX_LIGHTS."""
    lights = list(lights or ())
    if len(lights) > MAX_LIGHTS:
        raise ValueError("%d lights" % len(lights))
    return np.stack([record(**l) for l in lights]) if lights else np.zeros((0, 16), np.float32)


def sphere_sample(pixel, frame_index, i):
    """(o as three fp32, u, s) of step 5 for light i."""
    out = np.zeros(5, np.float32)
    lib().orc_light_sphere_sample(pixel, frame_index, i, _p(out))
    return out[:3].copy(), float(out[3]), int(out[4])


def figures(classes, aux):
    """The golden file's figures from [frames, lights, H, W] classes and [frames, lights, H, W, 2] (s, win): the first frame's class counts,
    per light the pixels lit in one frame and occluded in another, and -- first frame -- the pixels with terms of two lights or more, with
    a lit term inside the cone's falloff, with a lit term whose window is below one half."""
    n = classes.shape[1]
    lit0 = classes[0] == LIT
    return dict(classes=[[int((classes[0, i] == k).sum()) for k in range(7)] for i in range(n)],
                mixed=[int(((classes[:, i] == LIT).any(0) & (classes[:, i] == OCCLUDED).any(0)).sum()) for i in range(n)],
                two_lights=int((lit0.sum(0) >= 2).sum()),
                partial_cone=int((lit0 & (aux[0, ..., 0] > 0) & (aux[0, ..., 0] < 1)).any(0).sum()),
                window_below_half=int((lit0 & (aux[0, ..., 1] < 0.5)).any(0).sum()),
                light_rays=[int(x) for x in np.isin(classes, (OCCLUDED, LIT)).sum((1, 2, 3))])


def check_conditions(got, label):
    """The issue's conditions: every class 1-6 has 20 pixels for some light; 50 pixels lit in one frame and occluded in another for B or C;
    100 pixels with terms of two lights; 20 lit pixels with 0 < s < 1 and 20 with win < 0.5."""
    for k in range(1, 7):
        assert max(row[k] for row in got["classes"]) >= 20, (label, k, got)
    assert max(got["mixed"][1:]) >= 50 and got["two_lights"] >= 100 and got["partial_cone"] >= 20 and got["window_below_half"] >= 20, (label, got)


class Oracle(SS.Oracle):
    """SS.Oracle with lights.  light_classes: uint8 [count, H, W] of the last lights' pass; light_aux (statistics_lights on): float32
    [count, H, W, 2], s of the cone and the final win where a ray exists; light_rays: the pass's shadow rays."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256):
        self.depth, self.samples, self.sample_set = depth, samples, sample_set      # (SS.Oracle's, on this module's library)
        self.entry, self.taken = RS.ENTRIES["sampleset"]
        self.sun, self.sun_reflections = None, False
        self.force_sums = self.keep_counts = False
        self.classes = np.zeros((height, width), np.uint8)
        self.lit = np.zeros((height, width), np.uint8)
        self.counts = np.zeros((4, len(SS.SH.COLUMNS)), np.uint64)
        self.angle, self.statistics, self.primary_index, self.force_rule = 0.0, False, None, False
        self.centre = np.zeros((height, width), np.uint8)
        self.changed = np.zeros((height, width), np.uint8)
        self.soft = np.zeros((4, len(SS.SOFT_COLUMNS)), np.uint64)
        O.Oracle.__init__(self, width, height, threads, lib=lib())
        self.lights = np.zeros((0, 16), np.float32)
        self.light_classes = np.zeros((0, height, width), np.uint8)
        self.light_aux = np.zeros((0, height, width, 2), np.float32)
        self.statistics_lights = False
        self.light_rays = 0

    def set_lights(self, lights):
        """Refuses what the product refuses, keeping the lights."""
        self.lights = records(lights)

    def lights_apply(self, unoccluded=False):
        n = len(self.lights)
        H, W = self.classes.shape
        self.light_classes = np.zeros((n, H, W), np.uint8)
        self.light_aux = np.zeros((n, H, W, 2), np.float32)
        if n == 0:
            self.light_rays = 0
            return 0
        flat = np.ascontiguousarray(self.lights, np.float32)
        self.light_rays = int(self.L.orc_lights_apply_aux(self.h, _p(flat), n, self._frame_index(), _p(self.light_classes), 1 if unoccluded else 0,
                                                          _p(self.light_aux) if self.statistics_lights else None))
        return self.light_rays

    def ray_trace(self):
        rays = SS.Oracle.ray_trace(self)
        return rays + self.lights_apply()
