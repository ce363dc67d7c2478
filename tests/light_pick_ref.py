"""The CPU restatement of one shadow ray per surface point for all local lights (rtggx_set_light_sampling): tests/light_pick_ref.cpp --
tests/light_hit_ref.cpp, i.e. the whole oracle and every restatement below it, plus both passes of the new rule -- compiled on first use like
light_hit_ref.py's library; an Oracle with set_light_sampling whose ray_trace() runs the picking passes in mode 1 (and, with force_walker,
this module's copy of the path walker in mode 0); the draw's word in Python integers; the golden file's figures and conditions."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import light_hit_ref as LH
import lights_ref as LR
import restatement as RS
import sun_soft_ref as SS
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "light_pick_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "liblight_pick_ref.so")
# per level, of the touched hits: with a candidate, with two or more, the chosen ray's class (out_of_range: the target in the surface), the
# chosen light later than the first candidate without the fallback, the fallback, and per light the times it was chosen among two or more
COLUMNS = ("candidates", "two_candidates", "out_of_range", "below_horizon", "occluded", "lit", "later", "fallback") + tuple("chosen%d" % i for i in range(8))
PICK_SLOT = 96
NONE = 255      # info[..., 1] where no light was chosen
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
        for name, fn in list(vars(LH.lib()).items()):      # the signatures of everything below this library
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        u32, vp, f32 = C.c_uint32, C.c_void_p, C.c_float
        L.orc_light_pick_columns.restype, L.orc_light_pick_columns.argtypes = u32, []
        L.orc_light_pick_draw.restype, L.orc_light_pick_draw.argtypes = u32, [u32, u32, u32]
        L.orc_light_pick_apply.restype, L.orc_light_pick_apply.argtypes = C.c_uint64, [vp, vp, u32, u32, u32, vp, vp, vp, vp]
        L.orc_light_pick_intervals.restype, L.orc_light_pick_intervals.argtypes = None, [vp, vp]
        L.orc_ray_trace_light_pick.restype = C.c_uint64
        L.orc_ray_trace_light_pick.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, f32, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp]
        assert L.orc_light_pick_columns() == len(COLUMNS)
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def hit_slot(level, image):
    """The slot of the draw at a level-d hit of a path that writes image img."""
    return 104 + 2 * level + image


def draw_word(pixel, frame_index, slot):
    """v of the rule's step 3 from Python integers."""
    h = LH.rng((LH.rng(pixel) + frame_index) & 0xFFFFFFFF)
    return LH.rng((h + slot * 0x9E3779B9) & 0xFFFFFFFF)


def draw_word_lib(pixel, frame_index, slot):
    return int(lib().orc_light_pick_draw(pixel, frame_index, slot))


def luminance(rgb):
    """Y of the rule in float64, of [..., 3]."""
    rgb = np.asarray(rgb, np.float64)
    return 0.25 * rgb[..., 0] + 0.5 * rgb[..., 1] + 0.25 * rgb[..., 2]


def intervals(weights):
    """All 2^24 values of v >> 8 against eight weights (0: no candidate): per light (count, first, last) of the values that choose it."""
    w = np.ascontiguousarray(weights, np.float32).reshape(8)
    out = np.zeros((8, 3), np.uint64)
    lib().orc_light_pick_intervals(_p(w), _p(out))
    return [tuple(int(x) for x in row) for row in out]


class Oracle(LH.Oracle):
    """LH.Oracle with the mode.  Of the last frame's primary pass in mode 1: pick_info uint8 [H, W, 4] -- candidates, the chosen index (NONE),
    the class of the chosen ray (lights_ref's numbers; OUT_OF_RANGE: the target in the surface; 0: no candidate), flags (bit 0: the "none, so
    the last candidate" branch, bit 1: the chosen light is not the first candidate) --, pick_wf float32 [H, W, 2] (W, f), pick_terms float32
    [H, W, 6] (S0, S1 as added), pick_weights float32 [H, W, 8].  Of its hit passes: pick_counts uint64 [4, len(COLUMNS)] by level and
    pick_chosen0 int8 [2, H, W], the light chosen at the level-0 hit per image (-1: none).  unoccluded: every primary ray that exists
    counts as unoccluded.  force_walker: this module's walker is used in mode 0 as well."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256):
        self.depth, self.samples, self.sample_set = depth, samples, sample_set      # (LH.Oracle's, on this module's library)
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
        self.light_counts = np.zeros((4, 8, len(LH.COLUMNS)), np.uint64)
        self.light_lit = np.zeros((height, width), np.uint8)
        self.light_cls0 = np.zeros((8, 2, height, width), np.uint8)
        self.light_hit_rays = 0
        self.light_sampling, self.unoccluded = 0, False
        self.pick_info = np.zeros((height, width, 4), np.uint8)
        self.pick_wf = np.zeros((height, width, 2), np.float32)
        self.pick_terms = np.zeros((height, width, 6), np.float32)
        self.pick_weights = np.zeros((height, width, 8), np.float32)
        self.pick_counts = np.zeros((4, len(COLUMNS)), np.uint64)
        self.pick_chosen0 = np.full((2, height, width), -1, np.int8)

    def set_light_sampling(self, mode):
        """Refuses what the product refuses, keeping the setting."""
        if mode not in (0, 1) or isinstance(mode, bool):
            raise ValueError("mode %r" % (mode,))
        self.light_sampling = int(mode)

    def pick_count(self, name, level=None):
        a = self.pick_counts[:, COLUMNS.index(name)]
        return int((a if level is None else a[level:level + 1]).sum())

    def lights_apply(self, unoccluded=False):
        """LH.Oracle.lights_apply in mode 0; in mode 1 the picking pass."""
        if self.light_sampling != 1 or len(self.lights) == 0:
            self.pick_info[...] = 0
            self.pick_info[..., 1] = NONE
            self.pick_wf[...] = 0
            self.pick_terms[...] = 0
            self.pick_weights[...] = 0
            return LH.Oracle.lights_apply(self, unoccluded or self.unoccluded)
        n = len(self.lights)
        H, W = self.classes.shape
        self.light_classes = np.zeros((n, H, W), np.uint8)
        self.light_aux = np.zeros((n, H, W, 2), np.float32)
        flat = np.ascontiguousarray(self.lights, np.float32)
        index = self._frame_index() if self.primary_index is None else self.primary_index
        self.light_rays = int(self.L.orc_light_pick_apply(self.h, _p(flat), n, index, 1 if (unoccluded or self.unoccluded) else 0,
                                                          _p(self.pick_info), _p(self.pick_wf), _p(self.pick_terms), _p(self.pick_weights)))
        return self.light_rays

    def ray_trace(self):
        on = self.light_reflections and len(self.lights) > 0
        mode = self.light_sampling if on else 0
        if not (mode == 1 or self.force_walker):
            if not self.keep_counts:
                self.pick_counts[...] = 0
                self.pick_chosen0[...] = -1
            return LH.Oracle.ray_trace(self)
        sun_on = self.sun is not None and self.sun_reflections
        l, e = self.sun if self.sun is not None else (np.zeros(3, np.float32), np.zeros(3, np.float32))
        k, t, b = SS.disk(l, self.angle) if self.sun is not None else (np.float32(0.0), np.zeros(3, np.float32), np.zeros(3, np.float32))
        if not self.keep_counts:
            self.counts[...] = 0
            self.soft[...] = 0
            self.light_counts[...] = 0
            self.light_hit_rays = 0
            self.pick_counts[...] = 0
        lit, changed, llit, cls0 = np.zeros_like(self.lit), np.zeros_like(self.changed), np.zeros_like(self.light_lit), np.zeros_like(self.light_cls0)
        chosen0 = np.full_like(self.pick_chosen0, -1)
        flat = np.ascontiguousarray(self.lights, np.float32)
        flags = (1 if sun_on else 0) | (2 if self.force_sums else 0) | (4 if self.statistics and sun_on else 0) | (8 if on else 0)
        shadow = np.zeros(1, np.uint64)
        l, e = np.ascontiguousarray(l, np.float32), np.ascontiguousarray(e, np.float32)
        rays = int(self.L.orc_ray_trace_light_pick(self.h, self.depth, self.samples, self.sample_set, _p(l), _p(e), _p(t), _p(b), k, flags,
                                                   _p(self.counts), _p(lit), _p(self.soft), _p(changed),
                                                   _p(flat) if len(flat) else None, len(flat), _p(self.light_counts), _p(llit), _p(cls0), _p(shadow),
                                                   mode, _p(self.pick_counts), _p(chosen0)))
        self.lit = lit | self.lit if self.keep_counts else lit
        self.changed = changed | self.changed if self.keep_counts else changed
        self.light_lit = llit | self.light_lit if self.keep_counts else llit
        self.light_cls0 = np.maximum(cls0, self.light_cls0) if self.keep_counts else cls0
        self.pick_chosen0 = chosen0
        self.light_hit_rays = int(shadow[0]) + (self.light_hit_rays if self.keep_counts else 0)
        return rays + (self.sun_apply() if self.sun is not None else 0) + self.lights_apply()


def mapped_frame(o, blocks):
    """light_hit_ref.mapped_frame for an Oracle of this module."""
    o.pick_counts[...] = 0
    return LH.mapped_frame(o, blocks)


def record(o):
    """What figures() needs of a frame."""
    return o.pick_info.copy(), o.pick_counts.copy(), o.pick_chosen0.copy(), o.light_rays, o.light_hit_rays


def figures(frames, n, hits):
    """The golden file's figures from a list of record()s of one setting.  primary: over the frames, the pixel-frames with two candidates
    or more, per light the times it was chosen there, the pixels whose chosen light differs between two frames, the chosen rays by class,
    the chosen lights later than the first candidate without the fallback, and the shadow rays per frame.  hits (a setting with the
    lights at the hits): the same over the hits of all levels and samples, `differs` over the level-0 hits per (image, pixel)."""
    info = np.stack([f[0] for f in frames]).astype(np.int64)      # [frames, H, W, 4]
    two = info[..., 0] >= 2
    chosen = info[..., 1]
    some = chosen != NONE
    both = some[:, None] & some[None, :]
    out = dict(primary=dict(
        two_candidates=int(two.sum()), chosen=[int((two & (chosen == i)).sum()) for i in range(n)],
        differs=int(((chosen[:, None] != chosen[None, :]) & both).any((0, 1)).sum()),
        below_horizon=int((info[..., 2] == LR.BELOW_HORIZON).sum()), occluded=int((info[..., 2] == LR.OCCLUDED).sum()), lit=int((info[..., 2] == LR.LIT).sum()),
        later=int((((info[..., 3] & 1) == 0) & ((info[..., 3] & 2) != 0)).sum()), rays=[int(f[3]) for f in frames]))
    if hits:
        counts = np.stack([f[1] for f in frames]).astype(np.int64).sum((0, 1))      # over frames and levels
        ch0 = np.stack([f[2] for f in frames]).astype(np.int64)      # [frames, 2, H, W]
        s0 = ch0 >= 0
        out["hits"] = dict(
            two_candidates=int(counts[COLUMNS.index("two_candidates")]), chosen=[int(counts[COLUMNS.index("chosen%d" % i)]) for i in range(n)],
            differs=int(((ch0[:, None] != ch0[None, :]) & s0[:, None] & s0[None, :]).any((0, 1)).sum()),
            below_horizon=int(counts[COLUMNS.index("below_horizon")]), occluded=int(counts[COLUMNS.index("occluded")]), lit=int(counts[COLUMNS.index("lit")]),
            later=int(counts[COLUMNS.index("later")]), level1_lit=int(np.stack([f[1] for f in frames])[:, 1, COLUMNS.index("lit")].sum()),
            rays=[int(f[4]) for f in frames])
    return out


def check_conditions(got, label):
    """The issue's conditions, per pass: 100 with two candidates or more; every light chosen 20 times or more where it was not the only
    candidate; 50 whose chosen light differs between two frames; 20 chosen rays in each of below-horizon, occluded and lit; 20 where the
    chosen light is not the first candidate and the fallback branch was not needed."""
    for name, g in got.items():
        assert g["two_candidates"] >= 100, (label, name, g)
        assert min(g["chosen"]) >= 20, (label, name, g)
        assert g["differs"] >= 50, (label, name, g)
        assert min(g["below_horizon"], g["occluded"], g["lit"]) >= 20, (label, name, g)
        assert g["later"] >= 20, (label, name, g)
