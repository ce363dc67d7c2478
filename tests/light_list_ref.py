"""The CPU restatement of a light list beyond eight (rtggx_set_light_list): tests/light_list_ref.cpp -- tests/light_pick_ref.cpp, i.e. the
whole oracle and every restatement below it, plus mode 1's rule over ALL n lights of a list, without a cull, with the list's hash slots --
compiled on first use like light_pick_ref.py's library; an Oracle with set_light_list whose ray_trace() runs the list's passes; the cull
restated apart from the rule (per-block kept counts), with "in range at a pixel => kept" asserted on every frame computed; the slots in
Python integers; the golden file's figures and conditions."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import light_pick_ref as LP
import lights_ref as LR
import restatement as RS
import sun_soft_ref as SS
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "light_list_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "liblight_list_ref.so")
MAX_LIGHT_LIST = 1024
# per level, of the touched hits: with a candidate, with two or more, the chosen ray's class (out_of_range: the target in the surface), and
# the hits with two candidates or more whose chosen index is >= 8, the hits whose chosen index is >= 64
COLUMNS = ("candidates", "two_candidates", "out_of_range", "below_horizon", "occluded", "lit", "chosen_from_8", "chosen_from_64")
NONE = 0xFFFF      # info[..., 1] where no light was chosen
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
        for name, fn in list(vars(LP.lib()).items()):      # the signatures of everything below this library
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        u32, vp, f32 = C.c_uint32, C.c_void_p, C.c_float
        L.orc_light_list_columns.restype, L.orc_light_list_columns.argtypes = u32, []
        L.orc_light_list_slot.restype, L.orc_light_list_slot.argtypes = u32, [u32]
        L.orc_light_list_hit_slot.restype, L.orc_light_list_hit_slot.argtypes = u32, [u32, u32, u32]
        L.orc_light_list_apply.restype, L.orc_light_list_apply.argtypes = C.c_uint64, [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp]
        L.orc_light_list_cull.restype, L.orc_light_list_cull.argtypes = C.c_uint64, [vp, vp, u32, vp, vp, vp, vp, vp]
        L.orc_ray_trace_light_list.restype = C.c_uint64
        L.orc_ray_trace_light_list.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, f32, u32, vp, u32, vp, vp, vp]
        assert L.orc_light_list_columns() == len(COLUMNS)
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def slot(i):
    """The hash slot of light i's target at the primary surface, from Python integers."""
    return 16 + i if i < 8 else 4096 + i


def hit_slot(level, image, i):
    """The hash slot of light i's target at a level-d hit of a path that writes image img."""
    return 32 + 16 * level + 8 * image + i if i < 8 else 8192 + 1024 * (2 * level + image) + i


def records(lights):
    """[count, 16] fp32 of a sequence of dicts (lights_ref.record's arguments); ValueError on more than MAX_LIGHT_LIST."""
    lights = list(lights or ())
    if len(lights) > MAX_LIGHT_LIST:
        raise ValueError("%d lights" % len(lights))
    return np.stack([LR.record(**l) for l in lights]) if lights else np.zeros((0, 16), np.float32)


def casting(lights):
    """How many lights of a sequence of dicts have an intensity."""
    return sum(1 for l in lights if any(x > 0 for x in l["intensity"]))


class Oracle(LP.Oracle):
    """LP.Oracle with the list.  Of the last frame's primary pass with a list: list_info uint16 [H, W, 4] -- candidates, the chosen index
    (NONE), the class of the chosen ray (lights_ref's numbers; OUT_OF_RANGE: the target in the surface; 0: no candidate), flags (bit 0:
    the "none, so the last candidate" branch, bit 1: the chosen light is not the first candidate) --, list_wf float32 [H, W, 2] (W, f),
    list_terms float32 [H, W, 6] (S0, S1 as added), list_kept and list_cands uint32 [ceil(H/8), ceil(W/8)]: the cull's kept lights per
    block and the lights that are a candidate at some pixel of the block.  Of its hit passes: list_counts uint64 [4, len(COLUMNS)] by
    level and list_chosen0 int16 [2, H, W], the light chosen at the level-0 hit per image (-1: none).  Every primary pass asserts the
    implication the cull rests on: a casting light in range at a pixel of a block is kept for that block."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256):
        LP.Oracle.__init__(self, width, height, threads, depth=depth, samples=samples, sample_set=sample_set)
        self.L = lib()
        self.light_list = np.zeros((0, 16), np.float32)
        self.list_info = np.zeros((height, width, 4), np.uint16)
        self.list_info[..., 1] = NONE
        self.list_wf = np.zeros((height, width, 2), np.float32)
        self.list_terms = np.zeros((height, width, 6), np.float32)
        self.list_kept = np.zeros(((height + 7) // 8, (width + 7) // 8), np.uint32)
        self.list_cands = np.zeros_like(self.list_kept)
        self.list_counts = np.zeros((4, len(COLUMNS)), np.uint64)
        self.list_chosen0 = np.full((2, height, width), -1, np.int16)

    def set_light_list(self, lights):
        """Refuses what the product refuses, keeping what is held."""
        flat = records(lights)
        if len(flat) and len(self.lights):
            raise ValueError("a list beside lights")
        self.light_list = flat

    def set_lights(self, lights):
        flat = LR.records(lights)
        if len(flat) and len(self.light_list):
            raise ValueError("lights beside a list")
        self.lights = flat

    def list_count(self, name, level=None):
        a = self.list_counts[:, COLUMNS.index(name)]
        return int((a if level is None else a[level:level + 1]).sum())

    def lights_apply(self, unoccluded=False, sum_all=False):
        """LP.Oracle.lights_apply without a list; with one the list's primary pass and the cull's restatement.  sum_all: instead of the
        pick, list_terms receives the sum of every candidate's term behind a ray of its own; the images stay."""
        n = len(self.light_list)
        if n == 0:
            self.list_info[...] = 0
            self.list_info[..., 1] = NONE
            self.list_wf[...] = 0
            self.list_terms[...] = 0
            self.list_kept[...] = 0
            self.list_cands[...] = 0
            return LP.Oracle.lights_apply(self, unoccluded)
        H, W = self.classes.shape
        flat = np.ascontiguousarray(self.light_list, np.float32)
        index = self._frame_index() if self.primary_index is None else self.primary_index
        P = np.zeros((H, W, 3), np.float32)
        reach, cand = np.zeros((H, W, (n + 7) // 8), np.uint8), np.zeros((H, W, (n + 7) // 8), np.uint8)
        flags = (1 if (unoccluded or self.unoccluded) else 0) | (2 if sum_all else 0)
        rays = int(self.L.orc_light_list_apply(self.h, _p(flat), n, index, flags, _p(self.list_info), _p(self.list_wf), _p(self.list_terms), _p(P), _p(reach), _p(cand)))
        violations = int(self.L.orc_light_list_cull(self.h, _p(flat), n, _p(P), _p(reach), _p(cand), _p(self.list_kept), _p(self.list_cands)))
        assert violations == 0, "%d (block, light) pairs: in range at a pixel of the block and not kept" % violations
        assert (self.list_cands <= self.list_kept).all()
        self.list_P, self.list_reach, self.list_cand = P, reach, cand      # (what block_kept_chunks restates the cull from)
        if not sum_all:
            self.light_rays = rays
        return rays

    def ray_trace(self):
        n = len(self.light_list)
        if n == 0:
            if not self.keep_counts:
                self.list_counts[...] = 0
                self.list_chosen0[...] = -1
            return LP.Oracle.ray_trace(self)
        on = self.light_reflections
        sun_on = self.sun is not None and self.sun_reflections
        l, e = self.sun if self.sun is not None else (np.zeros(3, np.float32), np.zeros(3, np.float32))
        k, t, b = SS.disk(l, self.angle) if self.sun is not None else (np.float32(0.0), np.zeros(3, np.float32), np.zeros(3, np.float32))
        if not self.keep_counts:
            self.list_counts[...] = 0
            self.light_hit_rays = 0
        chosen0 = np.full_like(self.list_chosen0, -1)
        flat = np.ascontiguousarray(self.light_list, np.float32)
        flags = (1 if sun_on else 0) | (2 if self.force_sums else 0) | (8 if on else 0)
        shadow = np.zeros(1, np.uint64)
        l, e = np.ascontiguousarray(l, np.float32), np.ascontiguousarray(e, np.float32)
        rays = int(self.L.orc_ray_trace_light_list(self.h, self.depth, self.samples, self.sample_set, _p(l), _p(e), _p(t), _p(b), k, flags,
                                                   _p(flat), n, _p(shadow), _p(self.list_counts), _p(chosen0)))
        self.list_chosen0 = chosen0
        self.light_hit_rays = int(shadow[0]) + (self.light_hit_rays if self.keep_counts else 0)
        return rays + (self.sun_apply() if self.sun is not None else 0) + self.lights_apply()


def record(o):
    """What figures() needs of a frame."""
    return (o.list_info.copy(), o.list_counts.copy(), o.list_kept.copy(), o.list_cands.copy(), o.light_rays, o.light_hit_rays,
            block_covered(o.buffer(O.BUF_VISIBILITY) != 0))


def block_covered(covered):
    """[ceil(H/8), ceil(W/8)] bool of a [H, W] bool: the block has a covered pixel."""
    c = np.asarray(covered, bool)
    H, W = c.shape
    pad = np.zeros((-(-H // 8) * 8, -(-W // 8) * 8), bool)
    pad[:H, :W] = c
    return pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8).any((1, 3))


def block_kept_chunks(o):
    """Per block of the oracle's last primary pass with a list: does it keep a light of each 64-light chunk -- the cull restated once per
    chunk on the list with every light outside the chunk made dark.  -> bool [chunks, by, bx]."""
    n = len(o.light_list)
    out = []
    for c in range((n + 63) // 64):
        part = np.ascontiguousarray(o.light_list, np.float32).copy()
        part[:c * 64, 4:7] = 0
        part[(c + 1) * 64:, 4:7] = 0
        kept, cands = np.zeros_like(o.list_kept), np.zeros_like(o.list_cands)
        o.L.orc_light_list_cull(o.h, _p(part), n, _p(o.list_P), _p(o.list_reach), _p(o.list_cand), _p(kept), _p(cands))
        out.append(kept > 0)
    return np.stack(out)


def figures(frames, casting_lights, both_chunks, hits):
    """The golden file's figures from a list of record()s of one setting.  blocks, over the frames: with a covered pixel and nothing kept;
    with kept lights in both chunks (both_chunks: per frame a [by, bx] bool); whose kept count exceeds their candidates (the slack of a
    conservative test); with a covered pixel that keep fewer than a quarter of the casting lights; and the mean and the largest kept
    count over the blocks with a covered pixel.  primary: pixel-frames with two candidates or more and a chosen index >= 8; with a chosen
    index >= 64; the chosen rays by class; the shadow rays per frame.  hits: the same of the hits, all levels and samples."""
    info = np.stack([f[0] for f in frames]).astype(np.int64)      # [frames, H, W, 4]
    kept = np.stack([f[2] for f in frames]).astype(np.int64)
    cands = np.stack([f[3] for f in frames]).astype(np.int64)
    cov = np.stack([f[6] for f in frames])
    chosen = info[..., 1]
    some = chosen != NONE
    out = dict(blocks=dict(
        covered=int(cov.sum()), none_kept=int((cov & (kept == 0)).sum()), both_chunks=int(np.stack(both_chunks).sum()),
        slack=int((kept > cands).sum()), under_a_quarter=int((cov & (4 * kept < casting_lights)).sum()),
        kept_mean=float(kept[cov].mean()), kept_max=int(kept.max())),
        primary=dict(two_candidates_from_8=int(((info[..., 0] >= 2) & some & (chosen >= 8)).sum()), chosen_from_64=int((some & (chosen >= 64)).sum()),
                     below_horizon=int((info[..., 2] == LR.BELOW_HORIZON).sum()), occluded=int((info[..., 2] == LR.OCCLUDED).sum()), lit=int((info[..., 2] == LR.LIT).sum()),
                     rays=[int(f[4]) for f in frames]))
    if hits:
        counts = np.stack([f[1] for f in frames]).astype(np.int64)      # [frames, levels, columns]
        level0 = counts[:, 0].sum(0)
        out["hits"] = dict(two_candidates_from_8=int(level0[COLUMNS.index("chosen_from_8")]), chosen_from_64=int(level0[COLUMNS.index("chosen_from_64")]),
                           below_horizon=int(level0[COLUMNS.index("below_horizon")]), occluded=int(level0[COLUMNS.index("occluded")]), lit=int(level0[COLUMNS.index("lit")]),
                           rays=[int(f[5]) for f in frames])
    return out


# The conditions the golden list is chosen to meet, over its four frames.  The issue names the classes and leaves the numbers open: 8 blocks
# of each kind and 20 pixels or hits of each kind -- the bars tests/light_pick_ref.py uses for its classes (20), and a handful of blocks,
# enough that a wrong block index or chunk boundary cannot hide in one of them.
MIN_BLOCKS, MIN_POINTS = 8, 20


def check_conditions(got, label):
    b = got["blocks"]
    assert min(b["none_kept"], b["both_chunks"], b["slack"], b["under_a_quarter"]) >= MIN_BLOCKS, (label, b)
    for name in ("primary", "hits"):
        if name in got:
            g = got[name]
            assert min(g["two_candidates_from_8"], g["chosen_from_64"], g["below_horizon"], g["occluded"], g["lit"]) >= MIN_POINTS, (label, name, g)
