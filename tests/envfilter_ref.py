"""The CPU restatement of rtggx_prefilter_env (tests/envfilter_ref.cpp: the whole CPU oracle once, plus orc_prefilter_table and
orc_prefilter_env, written from the contract in include/rtggx.h), compiled on first use into tests/_build/ with the flags of
tests/restatement.py and in the same way.  The source cube C -- level 0 and the full box chain below it -- comes from
tests/envimage_ref.py; the taps are the oracle's environment().  Also the numpy float64 evaluation of the table's formulas and the float64
model of the whole sum (tests/env_ref.py's sampler, double accumulation) the host tests hold the restatement to."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import env_ref as R
import envimage_ref as E
import restatement
from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "envfilter_ref.cpp")
_OUT = os.path.join(_HERE, "_build", "libenvfilter_ref.so")

MIN_SAMPLES, MAX_SAMPLES, DEFAULT_SAMPLES = 64, 4096, 1024

_lib = None


def build():
    deps = [_SRC] + [os.path.join(O._HERE, f) for f in os.listdir(O._HERE) if f.endswith((".h", ".cpp"))]
    if os.path.exists(_OUT) and all(os.path.getmtime(d) <= os.path.getmtime(_OUT) for d in deps):
        return _OUT
    os.makedirs(os.path.dirname(_OUT), exist_ok=True)
    fd, tmp = tempfile.mkstemp(suffix=".so", dir=os.path.dirname(_OUT))
    os.close(fd)
    try:
        subprocess.check_call([os.environ.get("CXX", "g++")] + restatement._FLAGS + ["-shared", "-pthread", "-o", tmp, _SRC])
        os.replace(tmp, _OUT)      # (atomic: a concurrent first use sees the old library or the new one)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return _OUT


def lib():
    """The library, with the oracle's ctypes signatures (copied from the oracle's own loader) and the two functions'."""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        for name, fn in list(vars(O.lib()).items()):
            if name.startswith("orc_"):
                mine = getattr(L, name)
                mine.restype, mine.argtypes = fn.restype, fn.argtypes
        u32 = C.c_uint32
        L.orc_prefilter_table.restype, L.orc_prefilter_table.argtypes = u32, [u32, u32, u32, u32, C.c_void_p, C.POINTER(C.c_float)]
        L.orc_prefilter_env.restype, L.orc_prefilter_env.argtypes = C.c_int, [C.c_void_p, u32, C.c_void_p]
        _lib = L
    return _lib


def levels_of(size):
    return int(size).bit_length()      # floor(log2(size)) + 1


def table(S, M, m, N):
    """The restatement's sample table of level m: (float32 [K, 4] of (x, y, z, lod), invW as np.float32)."""
    t, inv = np.zeros((N, 4), np.float32), C.c_float()
    K = lib().orc_prefilter_table(S, M, m, N, t.ctypes.data_as(C.c_void_p), C.byref(inv))
    return t[:K].copy(), np.float32(inv.value)


def source_cube(level0_codes):
    """uint16 [6, S, S, 4] (RGBA16F codes of level 0) -> C as uint16 [texels, 4], mip-major: level 0 as it is and the box chain of its halves
    widened to fp32 (what rtggx_generate_env_mips leaves)."""
    level0_codes = np.ascontiguousarray(level0_codes, np.uint16)
    levels = E.chain(level0_codes[..., :3].copy().view(np.float16).astype(np.float32))
    return np.concatenate([level0_codes.reshape(-1, 4)] + ([E.pack(levels[1:])] if len(levels) > 1 else []))


def prefilter(level0_codes, N, threads=None):
    """RTGGX_BUF_ENV after rtggx_set_env of level 0 and rtggx_prefilter_env(N), restated: uint16 [texels, 4]."""
    S = level0_codes.shape[1]
    M = levels_of(S)
    src = source_cube(level0_codes)
    o = O.Oracle(1, 1, threads, lib=lib())
    try:
        o.set_env_rgba16f(S, M, src)
        out = np.zeros((src.shape[0], 4), np.uint16)
        assert lib().orc_prefilter_env(o.h, N, out.ctypes.data_as(C.c_void_p)) == 0
    finally:
        o.close()
    return out


# ---- float64 evaluations -------------------------------------------------------------------------------------------------------------------
def roughness(m, M):
    return min(1.0, 2.0 ** ((m - (M - 4)) / 1.15))


def table_float64(S, M, m, N):
    """The contract's formulas in numpy float64: (kept indices i, float64 [K, 4] of (x, y, z, lod))."""
    a2 = roughness(m, M) ** 4
    i = np.arange(N, dtype=np.uint64)
    rev = np.zeros(N, np.uint64)
    for b in range(32):
        rev |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    u = rev.astype(np.float64) / 4294967296.0
    c2 = (1.0 - u) / (1.0 + (a2 - 1.0) * u)
    z = 2.0 * c2 - 1.0
    keep = z > 0.0
    c2, z, k = c2[keep], z[keep], i[keep].astype(np.float64)
    phi = 2.0 * np.pi * k / N
    sin2 = 2.0 * np.sqrt(c2) * np.sqrt(1.0 - c2)
    d = (a2 - 1.0) * c2 + 1.0
    pdf = a2 / (np.pi * d * d) / 4.0
    lod = np.clip(0.5 * np.log2(6.0 * S * S / (4.0 * np.pi * N * pdf)) + 1.0, 0.0, M - 1.0)
    return i[keep].astype(np.int64), np.stack([sin2 * np.cos(phi), sin2 * np.sin(phi), z, lod], axis=1)


def _f32(*cols):
    return np.stack([np.asarray(c, np.float32) for c in cols], axis=-1)


def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross32(a, b):
    return _f32(a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0])


def _normalize32(v):
    inv = np.float32(1.0) / np.sqrt(_dot32(v, v))
    return v * inv[..., None]


def directions32(s, t32):
    """The directions the taps of a level of side s are taken in, as the contract computes them, operation by operation in np.float32:
    R = normalize(cubeFaceDir(f, u, v)) with u = ((float)x + 0.5f) / (float)s * 2.0f - 1.0f, then localToWorld(R, entry) -- up = +Y unless
    |R.y| >= 0.999, xAxis = normalize(cross(up, R)), yAxis = cross(R, xAxis), (xAxis l.x + yAxis l.y) + R l.z.  -> float32 [6 s s, K, 3]."""
    f32 = np.float32
    f, y, x = (a.reshape(-1) for a in np.meshgrid(np.arange(6), np.arange(s), np.arange(s), indexing="ij"))
    u = (x.astype(f32) + f32(0.5)) / f32(s) * f32(2.0) - f32(1.0)
    v = (y.astype(f32) + f32(0.5)) / f32(s) * f32(2.0) - f32(1.0)
    one = np.ones_like(u)
    faces = [_f32(one, -v, -u), _f32(-one, -v, u), _f32(u, one, v), _f32(u, -one, -v), _f32(u, -v, one), _f32(-u, -v, -one)]
    d = np.zeros((f.shape[0], 3), f32)
    for k in range(6):
        d[f == k] = faces[k][f == k]
    n = _normalize32(d)
    up = np.where((np.abs(n[:, 1]) < f32(0.999))[:, None], _f32(0.0, 1.0, 0.0), _f32(1.0, 0.0, 0.0)).astype(f32)
    xa = _normalize32(_cross32(up, n))
    ya = _cross32(n, xa)
    l = np.asarray(t32, f32)
    out = (xa[:, None, :] * l[None, :, 0:1] + ya[:, None, :] * l[None, :, 1:2]) + n[:, None, :] * l[None, :, 2:3]
    assert out.dtype == f32
    return out


def model(cube_levels, S, tables, inv_w):
    """The float64 model of the same sum for every texel of every level >= 1: `cube_levels` are the source cube C's levels (float64
    [6, s, s, 3] each), tables[m] the level's fp32 entries [K, 4] and inv_w[m] its fp32 invW, taken as they are; the taps' directions are the
    contract's fp32 ones (directions32); the sampler is tests/env_ref.py's and the accumulation is double.
    -> dict m -> (lo, hi) float64 [6, s, s, 3], the interval the sampler's corner taps leave open (lo == hi elsewhere)."""
    out = {}
    for m in range(1, len(cube_levels)):
        s = max(S >> m, 1)
        t = np.asarray(tables[m], np.float64)
        K = t.shape[0]
        d = directions32(s, tables[m][:, :3]).astype(np.float64).reshape(-1, 3)
        a, b = R.environment(cube_levels, S, d, np.tile(t[:, 3], 6 * s * s))
        w = np.tile(t[:, 2], 6 * s * s)[:, None]
        lo = (a * w).reshape(6 * s * s, K, 3).sum(axis=1) * float(inv_w[m])
        hi = (b * w).reshape(6 * s * s, K, 3).sum(axis=1) * float(inv_w[m])
        out[m] = (lo.reshape(6, s, s, 3), hi.reshape(6, s, s, 3))
    return out
