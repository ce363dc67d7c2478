"""Float64 models of the environment path, numpy only, written from the definitions and not from the kernels: the cube-map sampler
(D3D cube face selection, bilinear taps at texel centres, seamless edges, mip-linear blend with the shader's clamp rules) and the
projection of mip 0 onto nine spherical-harmonics coefficients.  They arbitrate between the HIP kernels (raytrace.hip environment(),
env.hip shProjectKernel) and the CPU oracle, which restate one another line by line (DESIGN.md "Tests").

Texels: `levels[m]` is a float64 array [6, s_m, s_m, 3] (face, row y, column x, rgb) with s_m = max(size >> m, 1).

The one thing the definitions leave open is a CORNER TAP: a bilinear tap whose x and y both lie outside the face.  D3D does not say which
texel it reads, and re-projecting its centre gives a direction with two components of equal magnitude, so rounding decides which of the two
neighbouring faces wins.  The model therefore returns an interval (lo, hi): per channel the smaller and the larger of the two neighbouring
faces' texels at that cube corner, carried through the (non-negative) bilinear and mip weights.  lo == hi wherever no corner tap takes
part."""
import numpy as np

# D3D cube map face selection (Direct3D 11 functional spec, "Cube map face selection"): the major axis picks the face, ties go to x, then
# y; per face (sc, tc, ma) with u = sc / |ma|, v = tc / |ma| in [-1, 1], u to the right and v down in the face's image.
# Rows: +x, -x, +y, -y, +z, -z; entries: (component, sign) of sc and of tc.
_SC = ((2, -1.0), (2, 1.0), (0, 1.0), (0, 1.0), (0, 1.0), (0, -1.0))
_TC = ((1, -1.0), (1, -1.0), (2, 1.0), (2, -1.0), (1, -1.0), (1, -1.0))
_AXIS = (0, 0, 1, 1, 2, 2)
_SIGN = (1.0, -1.0, 1.0, -1.0, 1.0, -1.0)


def face_uv(d):
    """d [n, 3] float64 -> (face [n] int, u [n], v [n])."""
    d = np.asarray(d, np.float64)
    a = np.abs(d)
    axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    n = np.arange(d.shape[0])
    face = 2 * axis + (d[n, axis] < 0.0)
    ma = a[n, axis]
    u = np.zeros(d.shape[0]); v = np.zeros(d.shape[0])
    for f in range(6):
        k = face == f
        u[k] = _SC[f][1] * d[k, _SC[f][0]] / ma[k]
        v[k] = _TC[f][1] * d[k, _TC[f][0]] / ma[k]
    return face, u, v


def face_dir(face, u, v):
    """The inverse of face_uv: the (unnormalised) direction through (u, v) of a face; |u|, |v| may exceed 1."""
    face = np.asarray(face)
    d = np.zeros((face.shape[0], 3))
    for f in range(6):
        k = face == f
        d[k, _AXIS[f]] = _SIGN[f]
        d[k, _SC[f][0]] = _SC[f][1] * u[k]      # sc = sign * component  =>  component = sign * sc
        d[k, _TC[f][0]] = _TC[f][1] * v[k]
    return d


def texel_centre_dirs(size):
    """Directions through the centres of every texel of a level of side `size`: (dirs [6 s s, 3], face, y, x)."""
    f, y, x = np.meshgrid(np.arange(6), np.arange(size), np.arange(size), indexing="ij")
    f, y, x = f.reshape(-1), y.reshape(-1), x.reshape(-1)
    return face_dir(f, (x + 0.5) / size * 2.0 - 1.0, (y + 0.5) / size * 2.0 - 1.0), f, y, x


def _edge_texel(tex, s, face, x, y):
    """A tap with at most ONE coordinate outside [0, s): inside the face its own texel; outside, the texel of the adjacent face that contains
    the direction through the tap's centre.  (That direction never lies on a texel border of the adjacent face: along the shared edge it falls
    at s (y + 1) / (s + 1), strictly between y and y + 1, and across it half a texel or less inside.)"""
    out = (x < 0) | (x >= s) | (y < 0) | (y >= s)
    f2, u2, v2 = face_uv(face_dir(face, (x + 0.5) / s * 2.0 - 1.0, (y + 0.5) / s * 2.0 - 1.0))
    x2 = np.clip(np.floor((u2 * 0.5 + 0.5) * s), 0, s - 1).astype(int)
    y2 = np.clip(np.floor((v2 * 0.5 + 0.5) * s), 0, s - 1).astype(int)
    return tex[np.where(out, f2, face), np.where(out, y2, np.clip(y, 0, s - 1)), np.where(out, x2, np.clip(x, 0, s - 1))]


def _tap(tex, s, face, x, y):
    """-> (lo, hi, corner): a tap's value as an interval; corner marks the taps with both coordinates outside the face."""
    ox, oy = (x < 0) | (x >= s), (y < 0) | (y >= s)
    corner = ox & oy
    # the two neighbouring faces' texels at the cube corner: the tap moved back inside along y, and along x
    a = _edge_texel(tex, s, face, x, np.where(corner, np.clip(y, 0, s - 1), y))
    b = _edge_texel(tex, s, face, np.where(corner, np.clip(x, 0, s - 1), x), y)
    return np.minimum(a, b), np.maximum(a, b), corner


def bilinear(tex, s, face, u, v):
    """One level, bilinear, taps at texel centres -> (lo, hi, corner [n] bool)."""
    x, y = (u * 0.5 + 0.5) * s - 0.5, (v * 0.5 + 0.5) * s - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    ix, iy = x0.astype(int), y0.astype(int)
    lo = np.zeros((u.shape[0], 3)); hi = np.zeros((u.shape[0], 3)); corner = np.zeros(u.shape[0], bool)
    for dx, dy, w in ((0, 0, (1.0 - fx) * (1.0 - fy)), (1, 0, fx * (1.0 - fy)), (0, 1, (1.0 - fx) * fy), (1, 1, fx * fy)):
        l, h, c = _tap(tex, s, face, ix + dx, iy + dy)
        lo += w[:, None] * l; hi += w[:, None] * h; corner |= c
    return lo, hi, corner


def level_split(level, mips):
    """The shader's level rule: clamp to [0, mips - 1]; the two levels blended and the weight of the second (0: the first alone)."""
    l = np.minimum(np.maximum(np.asarray(level, np.float64), 0.0), float(mips - 1))
    l0 = np.floor(l)
    m0 = l0.astype(int)
    return m0, np.minimum(m0 + 1, mips - 1), l - l0


def environment(levels, size, dir, level, with_corner=False):
    """The filtered cube map in directions dir [n, 3] at mip levels level [n] (or one for all) -> (lo, hi), each [n, 3] float64;
    with_corner: also the mask of directions in which a corner tap took part (lo == hi elsewhere)."""
    d = np.asarray(dir, np.float64).reshape(-1, 3)
    n = d.shape[0]
    mips = len(levels)
    m0, m1, fl = level_split(np.broadcast_to(np.asarray(level, np.float64), (n,)), mips)
    face, u, v = face_uv(d)
    lo = np.zeros((n, 3)); hi = np.zeros((n, 3)); corner = np.zeros(n, bool)
    for m in range(mips):
        s = max(size >> m, 1)
        assert levels[m].shape == (6, s, s, 3)
        ka, kb = m0 == m, (m1 == m) & (fl != 0.0)
        k = ka | kb
        if not k.any():
            continue
        l, h, c = bilinear(np.asarray(levels[m], np.float64), s, face[k], u[k], v[k])
        w = (np.where(ka[k], 1.0 - fl[k], 0.0) + np.where(kb[k], fl[k], 0.0))[:, None]      # m0 == m1 at the last level: both weights
        lo[k] += w * l; hi[k] += w * h; corner[k] |= c
    return (lo, hi, corner) if with_corner else (lo, hi)


# Real orthonormal spherical harmonics up to band 2 in the order the irradiance shader reads them (SHIrradianceTypeless.hlsli:16-37: L00,
# L1-1, L10, L11, L2-2, L2-1, L20, L21, L22), evaluated in the shader's frame (x, y, z) = (-d.x, -d.y, d.z).
def sh_basis(d):
    """d [n, 3] directions of the cube (any length) -> Y [n, 9] float64."""
    d = np.asarray(d, np.float64)
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    x, y, z = -d[:, 0], -d[:, 1], d[:, 2]
    k0, k1, k2, k3, k4 = 0.5 * np.sqrt(1.0 / np.pi), np.sqrt(3.0 / (4.0 * np.pi)), 0.5 * np.sqrt(15.0 / np.pi), 0.25 * np.sqrt(5.0 / np.pi), 0.25 * np.sqrt(15.0 / np.pi)
    return np.stack([np.full_like(x, k0), k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z, k3 * (3.0 * z * z - 1.0), k2 * x * z, k4 * (x * x - y * y)], axis=1)


def sh_project(level0, size):
    """The discrete projection of mip 0 ([6, size, size, 3]) -> (coeffs [9, 3], magnitude [9, 3]): sum over texels of Y_i(dir) w L with w the
    texel's solid angle up to a factor, 1 / |(u, v, 1)|^3, normalised so that the weights sum to 4 pi; magnitude is the same sum over
    |Y_i w L| -- what a rounding error of the sum is measured against."""
    L = np.asarray(level0, np.float64).reshape(6 * size * size, 3)
    d, _, _, _ = texel_centre_dirs(size)
    w = (d * d).sum(axis=1) ** -1.5
    Y = sh_basis(d)
    norm = 4.0 * np.pi / w.sum()
    T = Y[:, :, None] * (w[:, None] * L)[:, None, :]
    return T.sum(axis=0) * norm, np.abs(T).sum(axis=0) * norm
