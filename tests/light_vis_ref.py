"""The CPU restatement of the pick weighted by what the pixel remembers (rtggx_set_light_pick_visibility): tests/light_vis_ref.cpp --
tests/light_pick_ref.cpp, i.e. the whole oracle and every restatement below it, plus the primary pass with the records -- compiled on first
use like light_pick_ref.py's library; an Oracle that keeps the two record images, the sequence s and s0 across frames and takes a per-frame
camera (camera_frame); the update in Python integers; the class counts of a run of frames."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import light_pick_ref as LP
import lights_ref as LR
import restatement as RS
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "light_vis_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "liblight_vis_ref.so")
FLOOR = 16
RECORD = np.dtype([("v", np.uint8, 8), ("normal", np.uint32), ("stamp", np.uint32)])      # RtggxLightVisRecord
# vinfo[..., 0]: the history's class of a covered pixel
NOT_COVERED, VALID, SEQUENCE, OFF_FRAME, STAMP, INSTANCE, NORMAL = range(7)
INVALID = {"sequence": SEQUENCE, "off_frame": OFF_FRAME, "stamp": STAMP, "instance": INSTANCE, "normal": NORMAL}
# vinfo[..., 1]: a candidate below the floor; the pick is not mode 1's on the same draw; a candidate at 0; one at 255; a shadow ray was traced
F_FLOOR, F_DIFFERS, F_ZERO, F_FULL, F_UPDATED = 1, 2, 4, 8, 16
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
        u32, vp = C.c_uint32, C.c_void_p
        L.orc_light_vis_floor.restype, L.orc_light_vis_floor.argtypes = u32, []
        L.orc_light_vis_update.restype, L.orc_light_vis_update.argtypes = u32, [u32, u32]
        L.orc_light_vis_runs.restype, L.orc_light_vis_runs.argtypes = None, [vp]
        L.orc_light_vis_apply.restype, L.orc_light_vis_apply.argtypes = C.c_uint64, [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, u32, u32, vp]
        assert L.orc_light_vis_floor() == FLOOR
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def update(v, occluded):
    """Step 6 from Python integers."""
    return v - ((v + 3) >> 2) if occluded else v + ((255 - v + 3) >> 2)


def update_lib(v, occluded):
    return int(lib().orc_light_vis_update(v, 1 if occluded else 0))


def runs():
    """(occlusions in a row from 255 to 0, lit outcomes in a row from 0 to 255), counted by the restatement."""
    out = np.zeros(2, np.uint32)
    lib().orc_light_vis_runs(_p(out))
    return int(out[0]), int(out[1])


def weighted(w, v):
    """u of step 3 in fp32 from eight weights (0: no candidate) and eight bytes."""
    return (np.asarray(w, np.float32) * np.maximum(np.asarray(v, np.int64), FLOOR).astype(np.float32)).astype(np.float32)


class Oracle(LP.Oracle):
    """LP.Oracle with the setting.  images: RECORD [2, H, W], the two record images; seq, seq0: s and s0.  Of the last acting frame: vis_info
    uint8 [H, W, 4] -- the history's class, flags, the chosen light's byte before and after the update.  scramble: a callable (oracle) run in
    front of every acting frame's pass, behind s = s + 1 (the test that overwrites the image read)."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256):
        LP.Oracle.__init__(self, width, height, threads, depth, samples, sample_set)
        L = lib()      # (LP.Oracle creates its object on light_pick_ref's library: the same object once more, on this module's)
        self.L.orc_destroy(self.h)
        self.L = L
        self.h = C.c_void_p(L.orc_create(width, height))
        self.set_threads(threads if threads else min(os.cpu_count() or 1, 16))
        self.light_vis = False
        self.images = np.zeros((2, height, width), RECORD)
        self.allocated = False
        self.seq = self.seq0 = 0
        self.vis_info = np.zeros((height, width, 4), np.uint8)
        self.acted = False
        self.scramble = None

    def set_lights(self, lights):
        LP.Oracle.set_lights(self, lights)
        self.seq0 = self.seq

    def set_light_sampling(self, mode):
        LP.Oracle.set_light_sampling(self, mode)
        self.seq0 = self.seq

    def set_light_pick_visibility(self, enable):
        if enable not in (0, 1) or isinstance(enable, bool):
            raise ValueError("enable %r" % (enable,))
        if bool(enable) != self.light_vis:
            self.seq0 = self.seq
        self.light_vis = bool(enable)

    def acting(self):
        return self.light_vis and self.light_sampling == 1 and len(self.lights) > 0 and bool((np.asarray(self.lights, np.float32)[:, 4:7] > 0).any())

    def lights_apply(self, unoccluded=False):
        self.acted = self.acting()
        if not self.acted:
            self.vis_info[...] = 0
            return LP.Oracle.lights_apply(self, unoccluded)
        if not self.allocated:
            self.images[...] = 0
            self.allocated = True
            self.seq0 = self.seq
        self.seq += 1
        if self.scramble is not None:
            self.scramble(self)
        n = len(self.lights)
        H, W = self.classes.shape
        self.light_classes = np.zeros((n, H, W), np.uint8)
        self.light_aux = np.zeros((n, H, W, 2), np.float32)
        flat = np.ascontiguousarray(self.lights, np.float32)
        index = self._frame_index() if self.primary_index is None else self.primary_index
        self.light_rays = int(self.L.orc_light_vis_apply(self.h, _p(flat), n, index, 1 if (unoccluded or self.unoccluded) else 0,
                                                         _p(self.pick_info), _p(self.pick_wf), _p(self.pick_terms), _p(self.pick_weights),
                                                         _p(self.images[(self.seq - 1) & 1]), _p(self.images[self.seq & 1]), self.seq, self.seq0, _p(self.vis_info)))
        assert self.light_rays != 2 ** 64 - 1
        return self.light_rays

    def camera_frame(self, eye, dt=0.25, focus=(0.0, 3.0, 0.0)):
        """One frame under the camera at `eye`: the constants (the previous frame's matrices become this frame's history), the trees, the
        visibility pass, the traced images with every pass of the settings.  Returns the ray count."""
        self.update_frame(eye, O.camera_view_proj(self.W, self.H, eye, focus), dt)
        self.update_as(); self.render_visibility()
        return self.ray_trace()


def counts(o):
    """The class counts of the oracle's last acting frame, by name."""
    cls, flags, info = o.vis_info[..., 0], o.vis_info[..., 1].astype(int), o.pick_info.astype(int)
    some = info[..., 1] != LP.NONE
    out = {"valid": int((cls == VALID).sum())}
    out.update({k: int((cls == v).sum()) for k, v in INVALID.items()})
    out.update(floor=int(((flags & F_FLOOR) != 0).sum()), v0=int(((flags & F_ZERO) != 0).sum()), v255=int(((flags & F_FULL) != 0).sum()),
               lit=int((info[..., 2] == LR.LIT).sum()), occluded=int((info[..., 2] == LR.OCCLUDED).sum()),
               no_ray=int((some & ~np.isin(info[..., 2], (LR.LIT, LR.OCCLUDED))).sum()), differs=int(((flags & F_DIFFERS) != 0).sum()))
    return out


CLASSES = ("valid", "sequence", "off_frame", "stamp", "instance", "normal", "floor", "v0", "v255", "lit", "occluded", "no_ray", "differs")


def total(frames):
    return {k: sum(f[k] for f in frames) for k in CLASSES}


def check_conditions(frames, label):
    """The issue's class conditions over a run of frames: each count is non-zero."""
    t = total(frames)
    for k in CLASSES:
        assert t[k] > 0, (label, k, t)
