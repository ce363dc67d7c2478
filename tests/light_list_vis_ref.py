"""The CPU restatement of a list's pick weighted by what the pixel remembers (rtggx_set_light_list_visibility): tests/light_list_vis_ref.cpp
-- tests/light_list_ref.cpp, i.e. the whole oracle and every restatement below it, plus the list's primary pass with the sparse records over
ALL lights, without a cull -- compiled on first use like light_list_ref.py's library; an Oracle that keeps the two record images, the
sequence s and s0 across frames and takes a per-frame camera (camera_frame); the update in Python integers; the class counts of a run of
frames and the conditions the golden file's scene is chosen to meet."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import light_list_ref as LL
import lights_ref as LR
import restatement as RS
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "light_list_vis_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "liblight_list_vis_ref.so")
ENTRIES, FLOOR, FREE, FULL, INSERT = 4, 4, 0xFFFF, 63, 47
RECORD = np.dtype([("entry", np.uint16, 4), ("normal", np.uint32), ("stamp", np.uint32)])      # RtggxLightListVisRecord
# vinfo[..., 0]: the history's class of a covered pixel
NOT_COVERED, VALID, SEQUENCE, OFF_FRAME, STAMP, INSTANCE, NORMAL = range(7)
# vinfo[..., 1] & 15: what the update did -- no ray; the light has no entry and was seen; an entry's v moved; an entry was inserted into a
# free slot; it replaced an entry; an entry reached 63 and was freed
E_NONE, E_KEPT, E_MOVED, E_INSERTED, E_EVICTED, E_DROPPED = range(6)
# vinfo[..., 1]'s flags: a ray was traced; the carried record holds an entry; a candidate's v is below the floor; the pick is not the list's
F_RAY, F_CARRIED, F_FLOOR, F_DIFFERS = 16, 32, 64, 128
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
        for name, fn in list(vars(LL.lib()).items()):      # the signatures of everything below this library
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        u32, vp = C.c_uint32, C.c_void_p
        L.orc_light_list_vis_floor.restype, L.orc_light_list_vis_floor.argtypes = u32, []
        L.orc_light_list_vis_update.restype, L.orc_light_list_vis_update.argtypes = None, [vp, u32, u32, vp]
        L.orc_light_list_vis_apply.restype = C.c_uint64
        L.orc_light_list_vis_apply.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp]
        assert L.orc_light_list_vis_floor() == FLOOR
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def entry(v, light):
    return (v << 10) | light


def update(entries, light, occluded):
    """Step 6 from Python integers: (the four entries afterwards, the event, v before, v after)."""
    e = [int(x) for x in entries]
    slot = next((k for k in range(ENTRIES) if e[k] != FREE and (e[k] & 1023) == light), None)
    v = e[slot] >> 10 if slot is not None else FULL
    w = v - ((v + 3) >> 2) if occluded else v + ((FULL - v + 3) >> 2)
    if slot is not None:
        e[slot] = FREE if w == FULL else entry(w, light)
        return e, (E_DROPPED if w == FULL else E_MOVED), v, w
    if not occluded:
        return e, E_KEPT, v, w
    free = [k for k in range(ENTRIES) if e[k] == FREE]
    if free:
        e[free[0]] = entry(INSERT, light)
        return e, E_INSERTED, v, w
    most = max(x >> 10 for x in e)
    e[[x >> 10 for x in e].index(most)] = entry(INSERT, light)
    return e, E_EVICTED, v, w


def update_lib(entries, light, occluded):
    e, out = np.array(entries, np.uint16), np.zeros(3, np.uint32)
    lib().orc_light_list_vis_update(_p(e), light, 1 if occluded else 0, _p(out))
    return [int(x) for x in e], int(out[0]), int(out[1]), int(out[2])


class Oracle(LL.Oracle):
    """LL.Oracle with the setting.  images: RECORD [2, H, W], the two record images; seq, seq0: s and s0.  Of the last acting frame: vis_info
    uint8 [H, W, 4] -- the history's class, the update's event and flags, the chosen light's v before and after the update.  scramble: a
    callable (oracle) run in front of every acting frame's pass, behind s = s + 1 (the tests that overwrite the image read)."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256):
        LL.Oracle.__init__(self, width, height, threads, depth=depth, samples=samples, sample_set=sample_set)
        self.L = lib()
        self.list_vis = False
        self.images = np.zeros((2, height, width), RECORD)
        self.allocated = False
        self.seq = self.seq0 = 0
        self.vis_info = np.zeros((height, width, 4), np.uint8)
        self.acted = False
        self.scramble = None

    def set_light_list(self, lights):
        LL.Oracle.set_light_list(self, lights)
        self.seq0 = self.seq

    def set_light_list_visibility(self, enable):
        if enable not in (0, 1) or isinstance(enable, bool):
            raise ValueError("enable %r" % (enable,))
        if bool(enable) != self.list_vis:
            self.seq0 = self.seq
        self.list_vis = bool(enable)

    def acting(self):
        return self.list_vis and len(self.light_list) > 0 and bool((np.asarray(self.light_list, np.float32)[:, 4:7] > 0).any())

    def lights_apply(self, unoccluded=False, sum_all=False):
        self.acted = self.acting() and not sum_all
        if not self.acted:
            self.vis_info[...] = 0
            return LL.Oracle.lights_apply(self, unoccluded, sum_all)
        if not self.allocated:
            self.images[...] = 0
            self.allocated = True
            self.seq0 = self.seq
        self.seq += 1
        if self.scramble is not None:
            self.scramble(self)
        n = len(self.light_list)
        H, W = self.classes.shape
        flat = np.ascontiguousarray(self.light_list, np.float32)
        index = self._frame_index() if self.primary_index is None else self.primary_index
        P = np.zeros((H, W, 3), np.float32)
        reach, cand = np.zeros((H, W, (n + 7) // 8), np.uint8), np.zeros((H, W, (n + 7) // 8), np.uint8)
        rays = int(self.L.orc_light_list_vis_apply(self.h, _p(flat), n, index, 1 if (unoccluded or self.unoccluded) else 0, _p(self.list_info), _p(self.list_wf),
                                                   _p(self.list_terms), _p(P), _p(reach), _p(cand), _p(self.images[(self.seq - 1) & 1]), _p(self.images[self.seq & 1]),
                                                   self.seq, self.seq0, _p(self.vis_info)))
        assert rays != 2 ** 64 - 1
        violations = int(self.L.orc_light_list_cull(self.h, _p(flat), n, _p(P), _p(reach), _p(cand), _p(self.list_kept), _p(self.list_cands)))
        assert violations == 0, "%d (block, light) pairs: in range at a pixel of the block and not kept" % violations
        self.list_P, self.list_reach, self.list_cand = P, reach, cand
        self.light_rays = rays
        return rays

    def camera_frame(self, eye, dt=0.25, focus=(0.0, 3.0, 0.0)):
        """One frame under the camera at `eye`: the constants (the previous frame's matrices become this frame's history), the trees, the
        visibility pass, the traced images with every pass of the settings.  Returns the ray count."""
        self.update_frame(eye, O.camera_view_proj(self.W, self.H, eye, focus), dt)
        self.update_as(); self.render_visibility()
        return self.ray_trace()


CLASSES = ("valid", "sequence", "off_frame", "stamp_or_instance", "normal", "inserted", "evicted", "dropped", "reached_zero", "hidden_from_64",
           "no_ray_carried", "lit", "occluded", "floor", "differs")


def counts(o):
    """The class counts of the oracle's last acting frame, by name: pixel-frames with a valid history; with a history invalid for each of the
    four reasons; with an insert into a free slot, an eviction, an entry freed on reaching 63, an entry that reached 0; with a chosen light of
    index >= 64 whose v < 63; with a carried entry and no ray traced (the record is written as carried); the traced rays by outcome; pixels
    with a candidate below the floor; pixels whose pick is not the list's on the same draw."""
    cls, ev, info = o.vis_info[..., 0], o.vis_info[..., 1].astype(int), o.list_info.astype(int)
    before, after = o.vis_info[..., 2].astype(int), o.vis_info[..., 3].astype(int)
    event, ray, some = ev & 15, (ev & F_RAY) != 0, info[..., 1] != LL.NONE
    return dict(valid=int((cls == VALID).sum()), sequence=int((cls == SEQUENCE).sum()), off_frame=int((cls == OFF_FRAME).sum()),
                stamp_or_instance=int(((cls == STAMP) | (cls == INSTANCE)).sum()), normal=int((cls == NORMAL).sum()),
                inserted=int((event == E_INSERTED).sum()), evicted=int((event == E_EVICTED).sum()), dropped=int((event == E_DROPPED).sum()),
                reached_zero=int((ray & (event == E_MOVED) & (after == 0) & (before > 0)).sum()),
                hidden_from_64=int((some & (info[..., 1] >= 64) & (before < FULL)).sum()),
                no_ray_carried=int(((cls != NOT_COVERED) & ~ray & ((ev & F_CARRIED) != 0)).sum()),
                lit=int((info[..., 2] == LR.LIT).sum()), occluded=int((info[..., 2] == LR.OCCLUDED).sum()),
                floor=int(((ev & F_FLOOR) != 0).sum()), differs=int(((ev & F_DIFFERS) != 0).sum()))


def total(frames):
    return {k: sum(f[k] for f in frames) for k in CLASSES}


def check_conditions(frames, label):
    """The issue's class conditions over a run of frames: each count is non-zero."""
    t = total(frames)
    for k in CLASSES:
        assert t[k] > 0, (label, k, t)
