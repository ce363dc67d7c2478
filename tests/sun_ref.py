"""The CPU restatement of the sun (rtggx_set_sun): tests/sun_ref.cpp -- tests/restatements.cpp, i.e. the whole oracle and the depth, spp and
sample-set restatements, plus orc_sun_apply -- compiled on first use like restatement.py's library, with its flags; an Oracle whose ray_trace()
applies the sun behind the restatement it is set to; and the host's normalisation of the direction."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import restatement as RS
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "sun_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "libsun_ref.so")
NOT_COVERED, FACING_AWAY, OCCLUDED, LIT = 0, 1, 2, 3
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
        for name, fn in list(vars(RS.lib()).items()):      # the signatures of the oracle's and the restatements' functions
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        L.orc_sun_apply.restype, L.orc_sun_apply.argtypes = C.c_uint64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def normalise(direction):
    """The host's rule: the vector in double, divided by its length in double, rounded once to fp32."""
    d = np.asarray(direction, np.float32).astype(np.float64)
    return (d / np.sqrt((d * d).sum())).astype(np.float32)


class Oracle(RS.Oracle):
    """RS.Oracle whose ray_trace() is followed by the sun's pass while a sun is set; classes: the class map of the last frame."""

    def __init__(self, width, height, threads=None, depth=1, samples=1, sample_set=256, entry="sampleset"):
        self.depth, self.samples, self.sample_set = depth, samples, sample_set
        self.entry, self.taken = RS.ENTRIES[entry]
        self.sun = None
        self.classes = np.zeros((height, width), np.uint8)
        O.Oracle.__init__(self, width, height, threads, lib=lib())

    def set_sun(self, direction, irradiance):
        self.sun = None if direction is None else (normalise(direction), np.ascontiguousarray(irradiance, np.float32))
        if self.sun is not None and not (self.sun[1] > 0).any():
            self.sun = None

    def sun_apply(self):
        """Steps 1-5 on the oracle's RayTracingOut0/1 as they are; returns the number of shadow rays."""
        l, e = self.sun
        return int(self.L.orc_sun_apply(self.h, l.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), self.classes.ctypes.data_as(C.c_void_p)))

    def ray_trace(self):
        rays = RS.Oracle.ray_trace(self)
        return rays + (self.sun_apply() if self.sun is not None else 0)
