"""The CPU restatement of recursion depth D (rtggx_set_max_recursion_depth; include/rtggx.h, DESIGN.md "Recursion depth"): tests/recursion_ref.cpp
-- the whole CPU oracle (oracle/orc_capi.cpp) plus orc_ray_trace_depth -- compiled on first use with the oracle Makefile's flags into a
git-ignored library next to it, and an Oracle whose ray_trace() traces paths of that depth.  Everything else of the oracle (visibility,
denoiser, tone map) is its own code, unchanged."""
import ctypes as C
import os
import subprocess
import tempfile

from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "recursion_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "librecursion_ref.so")
_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-msse4.1", "-fPIC"]      # oracle/Makefile CXXFLAGS

_lib = None


def build():
    deps = [_SRC] + [os.path.join(O._HERE, f) for f in os.listdir(O._HERE) if f.endswith((".h", ".cpp"))]
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
    """The library, with the oracle's ctypes signatures (copied from the oracle's own loader) and orc_ray_trace_depth's."""
    global _lib
    if _lib is None:
        base = O.lib()
        L = C.CDLL(build())
        for name, fn in list(vars(base).items()):
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        L.orc_ray_trace_depth.restype = C.c_uint64
        L.orc_ray_trace_depth.argtypes = [C.c_void_p, C.c_uint32]
        _lib = L
    return _lib


class Oracle(O.Oracle):
    """O.Oracle on the restatement's library; ray_trace() traces paths of `depth` levels (1..4)."""

    def __init__(self, width, height, threads=None, depth=1):
        self.depth = depth
        L, O_lib = lib(), O._lib
        O._lib = L      # (O.Oracle.__init__ takes its library from O.lib())
        try:
            super().__init__(width, height, threads)
        finally:
            O._lib = O_lib

    def set_max_recursion_depth(self, depth):
        self.depth = int(depth)

    def ray_trace(self):
        return int(self.L.orc_ray_trace_depth(self.h, C.c_uint32(self.depth)))

    def ray_trace_depth1_oracle(self):
        """The oracle's own orc_ray_trace (raygen_pixel), for comparison with ray_trace() at depth 1."""
        return int(self.L.orc_ray_trace(self.h))
