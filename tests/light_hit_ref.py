"""The CPU restatement of the local lights at the surfaces the paths hit (rtggx_set_light_reflections): tests/light_hit_ref.cpp --
tests/lights_ref.cpp, i.e. the whole oracle, every restatement, the sun's passes and the lights' primary pass, plus
orc_ray_trace_light_hits -- compiled on first use like lights_ref.py's library; an Oracle with set_light_reflections whose ray_trace() walks
the paths through that function while the toggle is on and lights are set (or force_walker is), and through lights_ref's otherwise; the
hash slot in Python integers; the golden file's figures and conditions; and mapped_frame() for frames under a sample map."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import lights_ref as LR
import restatement as RS
import sun_soft_ref as SS
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "light_hit_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "liblight_hit_ref.so")
COLUMNS = ("out_of_range", "facing_away", "outside_cone", "below_horizon", "occluded", "lit", "lit_specular", "lit_diffuse")      # per level and light
CLASSES = COLUMNS[:6]
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
        for name, fn in list(vars(LR.lib()).items()):      # the signatures of everything below this library
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        u32, vp, f32 = C.c_uint32, C.c_void_p, C.c_float
        L.orc_light_hit_columns.restype, L.orc_light_hit_columns.argtypes = u32, []
        L.orc_light_hit_sample.restype, L.orc_light_hit_sample.argtypes = None, [u32, u32, u32, u32, u32, vp]
        L.orc_ray_trace_light_hits.restype = C.c_uint64
        L.orc_ray_trace_light_hits.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, f32, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
        assert L.orc_light_hit_columns() == len(COLUMNS)
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def rng(x):
    """The project's 32-bit hash (oracle/orc_raytrace.h rng) in Python integers."""
    x = (x * 747796405 + 1) & 0xFFFFFFFF
    x = (((x >> ((x >> 28) + 4)) ^ x) * 277803737) & 0xFFFFFFFF
    return ((x >> 22) ^ x) & 0xFFFFFFFF


def slot(level, image, light):
    """j of the rule."""
    return 32 + 16 * level + 8 * image + light


def sample_words(pixel, frame_index, level, image, light):
    """(w, u 65536, s) of the rule's step 2 from Python integers."""
    h = rng((rng(pixel) + frame_index) & 0xFFFFFFFF)
    w = rng((h + slot(level, image, light) * 0x9E3779B9) & 0xFFFFFFFF)
    return w, w & 0xFFFF, w >> 24


def sample_words_lib(pixel, frame_index, level, image, light):
    out = np.zeros(3, np.uint32)
    lib().orc_light_hit_sample(pixel, frame_index, level, image, light, _p(out))
    return tuple(int(x) for x in out)


class Oracle(LR.Oracle):
    """LR.Oracle with the toggle.  Of the last frame: light_counts uint64 [4, 8, len(COLUMNS)] by level and light; light_lit uint8 [H, W], bit
    0 / 1 where a light's term exists in RayTracingOut0 / 1 (lit: a term of either feature); light_cls0 uint8 [8, 2, H, W], the class
    (lights_ref's numbers, 0: no touched hit) of the level-0 hit per light and image; light_hit_rays: the shadow rays from hits under the
    lights.  force_walker: the new walker is used with the toggle off or without lights as well."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256):
        self.depth, self.samples, self.sample_set = depth, samples, sample_set      # (LR.Oracle's, on this module's library)
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
        self.light_reflections, self.force_walker = False, False
        self.light_counts = np.zeros((4, 8, len(COLUMNS)), np.uint64)
        self.light_lit = np.zeros((height, width), np.uint8)
        self.light_cls0 = np.zeros((8, 2, height, width), np.uint8)
        self.light_hit_rays = 0

    def set_light_reflections(self, on):
        """Refuses what the product refuses, keeping the setting."""
        if on not in (0, 1, False, True):
            raise ValueError("enable %r" % (on,))
        self.light_reflections = bool(on)

    def light_count(self, name, level=None, light=None):
        a = self.light_counts[..., COLUMNS.index(name)]
        a = a if level is None else a[level:level + 1]
        a = a if light is None else a[:, light:light + 1]
        return int(a.sum())

    def lights_apply(self, unoccluded=False):
        """LR.Oracle.lights_apply, drawing with the frame's own index in a part of a mapped frame (primary_index)."""
        n = len(self.lights)
        H, W = self.classes.shape
        self.light_classes = np.zeros((n, H, W), np.uint8)
        self.light_aux = np.zeros((n, H, W, 2), np.float32)
        if n == 0:
            self.light_rays = 0
            return 0
        flat = np.ascontiguousarray(self.lights, np.float32)
        index = self._frame_index() if self.primary_index is None else self.primary_index
        self.light_rays = int(self.L.orc_lights_apply_aux(self.h, _p(flat), n, index, _p(self.light_classes), 1 if unoccluded else 0,
                                                          _p(self.light_aux) if self.statistics_lights else None))
        return self.light_rays

    def ray_trace(self):
        on = self.light_reflections and len(self.lights) > 0
        if not (on or self.force_walker):
            if not self.keep_counts:
                self.light_counts[...] = 0
                self.light_lit[...] = 0
                self.light_cls0[...] = 0
                self.light_hit_rays = 0
            return LR.Oracle.ray_trace(self)
        sun_on = self.sun is not None and self.sun_reflections
        l, e = self.sun if self.sun is not None else (np.zeros(3, np.float32), np.zeros(3, np.float32))
        k, t, b = SS.disk(l, self.angle) if self.sun is not None else (np.float32(0.0), np.zeros(3, np.float32), np.zeros(3, np.float32))
        if not self.keep_counts:
            self.counts[...] = 0
            self.soft[...] = 0
            self.light_counts[...] = 0
            self.light_hit_rays = 0
        lit, changed, llit, cls0 = np.zeros_like(self.lit), np.zeros_like(self.changed), np.zeros_like(self.light_lit), np.zeros_like(self.light_cls0)
        flat = np.ascontiguousarray(self.lights, np.float32)
        flags = (1 if sun_on else 0) | (2 if self.force_sums else 0) | (4 if self.statistics and sun_on else 0) | (8 if on else 0)
        shadow = np.zeros(1, np.uint64)
        l, e = np.ascontiguousarray(l, np.float32), np.ascontiguousarray(e, np.float32)
        rays = int(self.L.orc_ray_trace_light_hits(self.h, self.depth, self.samples, self.sample_set, _p(l), _p(e), _p(t), _p(b), k, flags,
                                                   _p(self.counts), _p(lit), _p(self.soft), _p(changed),
                                                   _p(flat) if len(flat) else None, len(flat), _p(self.light_counts), _p(llit), _p(cls0), _p(shadow)))
        self.lit = lit | self.lit if self.keep_counts else lit
        self.changed = changed | self.changed if self.keep_counts else changed
        self.light_lit = llit | self.light_lit if self.keep_counts else llit
        self.light_cls0 = np.maximum(cls0, self.light_cls0) if self.keep_counts else cls0
        self.light_hit_rays = int(shadow[0]) + (self.light_hit_rays if self.keep_counts else 0)
        return rays + (self.sun_apply() if self.sun is not None else 0) + self.lights_apply()


def figures(o_frames, n=8):
    """The golden file's figures from a list of per-frame (light_counts, light_cls0, light_hit_rays) of one setting: per light the level-0
    class counts of the first frame, the lit hits by lobe, the pixels with terms of two or more lights in one image, per light the level-0
    hits lit in one frame and occluded in another, level 1's lit and occluded hits, and the shadow rays from hits per frame."""
    counts0, cls_first, _ = o_frames[0]
    cls = np.stack([f[1] for f in o_frames])      # [frames, 8, 2, H, W]
    lit = cls == LR.LIT
    return dict(level0=[[int(counts0[0, i, k]) for k in range(len(COLUMNS))] for i in range(n)],
                lit_specular=int(counts0[0, :, COLUMNS.index("lit_specular")].sum()), lit_diffuse=int(counts0[0, :, COLUMNS.index("lit_diffuse")].sum()),
                two_lights=int(((cls_first == LR.LIT).sum(0) >= 2).any(0).sum()),
                mixed=[int((lit[:, i].any(0) & (cls[:, i] == LR.OCCLUDED).any(0)).sum()) for i in range(n)],
                level1=[int(counts0[1, :, COLUMNS.index(k)].sum()) for k in ("lit", "occluded")],
                hit_rays=[int(f[2]) for f in o_frames])


def check_conditions(got, radii, label, depth=1):
    """The issue's conditions.  Level 0: every class has 20 hits for some light; 20 lit hits per lobe; 50 pixels with terms of two or more
    lights in one image; 20 hits of a light with a radius lit in one frame and occluded in another.  Level 1 of a depth >= 2 frame: 20 lit
    and 20 occluded hits."""
    for k in range(len(CLASSES)):
        assert max(row[k] for row in got["level0"]) >= 20, (label, CLASSES[k], got)
    assert got["lit_specular"] >= 20 and got["lit_diffuse"] >= 20, (label, got)
    assert got["two_lights"] >= 50, (label, got)
    assert max([m for m, r in zip(got["mixed"], radii) if r > 0] or [0]) >= 20, (label, got)
    if depth >= 2:
        assert min(got["level1"]) >= 20, (label, got)


def mapped_frame(o, blocks):
    """sun_soft_ref.mapped_frame for an Oracle of this module."""
    o.light_counts[...] = 0
    o.light_lit[...] = 0
    o.light_cls0[...] = 0
    o.light_hit_rays = 0
    return SS.mapped_frame(o, blocks)
