"""Synthetic cube maps, direction sets and mip levels shared by tests/test_env_ref_host.py (model against the oracle) and
tests/test_gpu_env.py (HIP kernels against both).  Everything is generated from seeds; nothing is read from a file."""
import functools

import numpy as np

import env_ref as R

# (size, mips): 1x1; the smallest chain; odd and even sides that are no power of two (where (x + 0.5) / s * 2 - 1 rounds in fp32), with
# last levels of side 1, 2 and 3; one level only (every roughness clamps to level 0); a power of two with a full chain.
SHAPES = ((1, 1), (2, 2), (3, 2), (5, 3), (6, 3), (7, 1), (12, 3), (16, 5))
SPECIAL = (6, 3)          # ... and this shape once more with negative values, half denormals, 65504 and both zeros
N_DIRS = 4096
EPS = 2.0 ** -24          # unit roundoff of fp32


def side(size, m):
    return max(size >> m, 1)


class Cube:
    """Texels as RGBA16F codes per level: codes[m] is uint16 [6, s, s, 4]."""

    def __init__(self, size, mips, codes, name):
        self.size, self.mips, self.codes, self.name = size, mips, codes, name
        self.levels = [c[..., :3].view(np.float16).astype(np.float64) for c in codes]

    def mip_major(self):
        """uint16 [texels, 4], mip-major with six faces per mip: the oracle's input and the layout of the decoded environment."""
        return np.concatenate([c.reshape(-1, 4) for c in self.codes])

    def dds_order(self):
        """uint16, per face its whole mip chain: the layout of a DDS file, which rtggx_set_env takes."""
        return np.concatenate([self.codes[m][f].reshape(-1) for f in range(6) for m in range(self.mips)])


def random_cube(size, mips, seed=None):
    rng = np.random.default_rng(1000 * size + mips if seed is None else seed)
    codes = []
    for m in range(mips):
        s = side(size, m)
        t = rng.uniform(0.0, 8.0, (6, s, s, 4)).astype(np.float16)
        t[..., 3] = 1.0
        codes.append(t.view(np.uint16).copy())
    return Cube(size, mips, codes, "%dx%d_%dmips" % (size, size, mips))


def special_cube(largest=True):
    """SPECIAL with signed values, half denormals (codes 1 ... 0x3FF, both signs), 65504, -65504 and +-0 among ordinary texels.
    largest=False: without the +-65504 texels.  They make M and D of the bound 65504 and 131008, so that the model can only see gross
    errors on that cube; the same signed, denormal and zero texels without them are held to a B of 1e-5."""
    size, mips = SPECIAL
    rng = np.random.default_rng(77)
    codes = []
    for m in range(mips):
        s = side(size, m)
        t = rng.uniform(-2.0, 8.0, (6, s, s, 4)).astype(np.float16).view(np.uint16).copy()
        kind = rng.integers(0, 10, (6, s, s, 3))
        den = rng.integers(1, 0x400, (6, s, s, 3)).astype(np.uint16) | (rng.integers(0, 2, (6, s, s, 3)).astype(np.uint16) << 15)
        rgb = t[..., :3]
        rgb[kind == 0] = den[kind == 0]
        rgb[kind == 1] = 0x0000
        rgb[kind == 2] = 0x8000
        t[..., 3] = 0x3C00
        codes.append(t)
    # the largest finite half, with either sign, on every level: in a face's interior, on an edge and in a corner
    for m in range(mips if largest else 0):
        s = side(size, m)
        codes[m][0, 0, 0, 0] = 0x7BFF; codes[m][5, s - 1, s - 1, 1] = 0xFBFF; codes[m][2, s // 2, 0, 2] = 0x7BFF; codes[m][3, s // 2, s // 2, 0] = 0x7BFF
    return Cube(size, mips, codes, "%dx%d_%dmips_%s" % (size, size, mips, "special" if largest else "signed"))


def all_cubes():
    return [random_cube(s, m) for s, m in SHAPES] + [special_cube(), special_cube(largest=False)]


class Directions:
    """d: float32 [N_DIRS, 3]; the slices name what each part was built for."""

    def __init__(self, d, parts):
        self.d, self.parts = d, parts

    def part(self, name):
        a, b = self.parts[name]
        return slice(a, b)


def _signs():
    return np.array([[sx, sy, sz] for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)])


def directions(size, seed=5):
    """About 4096 directions for a cube of side `size`: the six axes; exact ties of two and of three magnitudes; two magnitudes equal to within
    1e-7 ... 1e-1 relative (cube edges) and three (cube corners), in every sign combination and every order of the axes; the centres of
    level 0's texels (scaled by powers of two, which keeps them exact); random normal vectors; lengths from 1e-3 to 1e3.  No zero, NaN or
    infinite vector: the sampler's float-to-int conversion is undefined for those."""
    rng = np.random.default_rng(seed + 31 * size)
    sg = _signs()
    perms = np.array([[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]])
    chunks, parts, at = [], {}, 0

    def add(name, a):
        nonlocal at
        a = np.asarray(a, np.float64).reshape(-1, 3)
        chunks.append(a); parts[name] = (at, at + a.shape[0]); at += a.shape[0]

    def spread(base):
        """every sign combination and order of the axes of each row, cycling"""
        n = base.shape[0]
        p = perms[np.arange(n) % 6]
        out = np.take_along_axis(base, np.argsort(p, axis=1), axis=1)
        return out * sg[(np.arange(n) // 6) % 8]

    add("axes", np.concatenate([np.eye(3), -np.eye(3)]))
    # exact ties: (1, 1, t) with t below, equal to and above 1
    t = np.concatenate([rng.uniform(0.0, 1.0, 32), np.ones(48), rng.uniform(1.0, 3.0, 16)])
    add("ties", spread(np.repeat(np.stack([np.ones(96), np.ones(96), t], axis=1), 4, axis=0)))
    n_edge = 720
    rel = 10.0 ** rng.uniform(-7.0, -1.0, n_edge) * rng.choice([-1.0, 1.0], n_edge)
    add("edges", spread(np.stack([np.ones(n_edge), 1.0 + rel, rng.uniform(0.0, 1.0, n_edge)], axis=1)))
    n_corner = 528
    r1 = 10.0 ** rng.uniform(-7.0, -1.0, n_corner) * rng.choice([-1.0, 1.0], n_corner)
    r2 = 10.0 ** rng.uniform(-7.0, -1.0, n_corner) * rng.choice([-1.0, 1.0], n_corner)
    add("corners", spread(np.stack([np.ones(n_corner), 1.0 + r1, 1.0 + r2], axis=1)))
    c, _, _, _ = R.texel_centre_dirs(size)
    c = c * 2.0 ** rng.integers(-10, 11, c.shape[0])[:, None]
    add("centres", c)
    n_rand = N_DIRS - at
    add("random", rng.standard_normal((n_rand, 3)))
    d = np.concatenate(chunks)
    # lengths 1e-3 ... 1e3 for everything but the texel centres, whose components must stay exact
    scale = 10.0 ** rng.uniform(-3.0, 3.0, d.shape[0])
    a, b = parts["centres"]
    scale[a:b] = 1.0
    scale[:6] = (1.0, 1e-3, 1e3, 1.0, 1e3, 1e-3)
    d32 = (d * scale[:, None]).astype(np.float32)
    assert d32.shape == (N_DIRS, 3) and np.isfinite(d32).all() and (np.abs(d32).max(axis=1) > 0).all()
    return Directions(d32, parts)


def special_levels(mips):
    """Every integer level and its two fp32 neighbours, -1, -0.0, mips - 1 and mips + 0.5."""
    out = [-1.0, -0.0, float(mips - 1), mips + 0.5]
    for m in range(mips):
        f = np.float32(m)
        out += [f, np.nextafter(f, np.float32(-1e9)), np.nextafter(f, np.float32(1e9))]
    return np.array(out, np.float32)


def levels_for(mips, n=N_DIRS, seed=9):
    """One level per direction: the special ones cycled through one half (shuffled), fractional levels over the chain in the other."""
    rng = np.random.default_rng(seed + mips)
    sp = special_levels(mips)
    lv = np.where(rng.random(n) < 0.5, sp[rng.integers(0, sp.size, n)], rng.uniform(-0.25, mips - 0.75, n).astype(np.float32))
    lv[:sp.size] = sp          # each at least once, on directions of the first parts
    lv[-sp.size:] = sp         # ... and on random ones
    return lv.astype(np.float32)


def bound(cube, level):
    """B: what a faithful fp32 evaluation of the sampler (every operation rounded once, in any sensible order) may differ from the exact
    value by, per direction.  With eps = 2^-24, s the side of the finer of the two levels blended, and over the texels of those two levels
    (of the one, where the weight of the second is 0) M = max |texel| and D = max texel - min texel:
      position   u = sc / ma: eps.  t = u / 2 + 1 / 2: eps / 2 carried + eps.  t * s: 1.5 eps s carried + eps s.  - 0.5: eps s.  The tap
                 position x is off by at most 3.5 eps s, the fraction fx = x - floor(x) by one rounding more (eps): 3.5 eps s + eps, and the
                 same for y.  The filtered value is a continuous, piecewise bilinear function of (x, y) -- across a floor() step the tap set
                 shifts by one and the weights swap 0 and 1 -- with slope at most D per texel in each coordinate: (7 s + 2) eps D.
      weights    1 - fx and 1 - fy: eps each; their product: eps.  At most 3 eps per weight, four weights, times M: 12 eps M.
      sum        four products (eps times a weight each, the weights sum to 1: eps M) and three additions (eps M each): 4 eps M.
      mip blend  1 - fl: eps; two products and one addition: 4 eps M together.  (fl itself is exact: level - floor(level) below 16.)
    B = ((7 s + 2) D + 20 M) eps.  Texel fetches are exact (binary16 -> fp32), an edge tap's re-projection cannot change its texel (it lands
    at least 1 / (s + 1) of a texel from a border), and a corner tap's choice is inside the model's interval by construction."""
    m0, m1, fl = R.level_split(level, cube.mips)
    m1 = np.where(fl != 0.0, m1, m0)
    s = np.maximum(cube.size >> m0, 1).astype(np.float64)
    hi, lo = np.array([l.max() for l in cube.levels]), np.array([l.min() for l in cube.levels])
    D = np.maximum(hi[m0], hi[m1]) - np.minimum(lo[m0], lo[m1])
    M = np.maximum(np.maximum(np.abs(hi[m0]), np.abs(lo[m0])), np.maximum(np.abs(hi[m1]), np.abs(lo[m1])))
    return ((7.0 * s + 2.0) * D + 20.0 * M) * EPS


# ---- SH ----------------------------------------------------------------------------------------------------------------------------------
SH_SIZES = (1, 2, 3, 7, 16, 33)      # 6 s^2 = 6, 24, 54 (less than one workgroup), 294 (one and a part), 1536 (six exactly), 6534 (25 and a part)
SH_BOUND = 2.0 ** -23                # times magnitude: one fp32 rounding of the result (2^-24) and as much again for every fp64 step before it


def sh_cube(size, seed=None):
    """One level of signed radiance in [-2, 8), RGBA16F codes [6, s, s, 4]."""
    rng = np.random.default_rng(500 + size if seed is None else seed)
    t = rng.uniform(-2.0, 8.0, (6, size, size, 4)).astype(np.float16)
    t[..., 3] = 1.0
    return Cube(size, 1, [t.view(np.uint16).copy()], "sh_%d" % size)


def constant_cube(size, value=1.0):
    t = np.full((6, size, size, 4), value, np.float16)
    return Cube(size, 1, [t.view(np.uint16).copy()], "const_%d" % size)


def basis_cube(size, k):
    """Basis function Y_k at the texel centres, rounded to binary16 (the cube's texel format)."""
    d, _, _, _ = R.texel_centre_dirs(size)
    y = R.sh_basis(d)[:, k].reshape(6, size, size)
    t = np.ones((6, size, size, 4), np.float16)
    t[..., :3] = y[..., None].astype(np.float16)
    return Cube(size, 1, [t.view(np.uint16).copy()], "Y%d_%d" % (k, size))


@functools.lru_cache(maxsize=None)
def basis_answer(k, size=64):
    """(coefficients of the float64 cube Y_k, the discretisation error allowed) -- the 64 x 64 midpoint rule's error falls with the
    square of the texel size, so it is 4/3 of the distance to the 128-cube's result to leading order; twice that is allowed."""
    out = []
    for s in (size, 2 * size):
        d, _, _, _ = R.texel_centre_dirs(s)
        y = R.sh_basis(d)[:, k].reshape(6, s, s, 1).repeat(3, axis=3)
        out.append(R.sh_project(y, s)[0])
    return out[0], 2.0 * (4.0 / 3.0) * np.abs(out[0] - out[1]) + 1e-12


def oracle_environment(o, dirs, levels):
    """oracle.Oracle.environment over a direction set -> float32 [n, 3]."""
    lv = np.broadcast_to(np.asarray(levels, np.float32), (dirs.shape[0],))
    return np.stack([o.environment(d, float(l)) for d, l in zip(dirs, lv)]).astype(np.float32)
