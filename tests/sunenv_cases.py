"""Synthetic cubes for the sun from the environment (tests/test_sunenv_host.py, tests/test_gpu_sunenv.py): a constant or smoothly varying
background in binary16 plus a patch of bright texels about a peak at a face centre, at the middle of an edge (the cone spans two faces) or
in a corner (three), on each of the six faces; and the special ones -- a plateau of equal maxima, texels holding NaN, +inf and negatives,
a constant cube, a black cube, and the degenerate sides 1, 2, 3, 5.  Everything is generated from seeds; nothing is read from a file.

A case is a level 0 as RGBA16F codes uint16 [6, S, S, 4] and the arguments of the call."""
import numpy as np

import sunenv_ref as SR

PLACES = ("centre", "edge", "corner")
FACES_IN_CONE = {"centre": 1, "edge": 2, "corner": 3}


class Case:
    def __init__(self, name, codes, cone=0.0, ring=0.0, min_contrast=0.0, faces=None, peak=None):
        self.name, self.codes, self.cone, self.ring, self.min_contrast = name, np.ascontiguousarray(codes, np.uint16), cone, ring, min_contrast
        self.faces, self.peak = faces, peak      # what the case was built to have: faces the cone touches, (face, x, y) of the peak
        self.S = self.codes.shape[1]

    @property
    def args(self):
        return dict(cone=self.cone, ring=self.ring, min_contrast=self.min_contrast)

    def __repr__(self):
        return self.name


def peak_texel(S, place):
    """(x, y) of the peak on its face: the centre, the middle of the edge x = S - 1, the corner (S - 1, S - 1)."""
    return {"centre": (S // 2, S // 2), "edge": (S - 1, S // 2), "corner": (S - 1, S - 1)}[place]


def background(S, smooth, seed):
    """float64 [6 S^2, 3] in about [0.2, 1.5]: constant, or a low-order function of the direction (no texel anywhere near the sun's level)."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.4, 1.0, 3)
    if not smooth:
        return np.tile(base, (6 * S * S, 1))
    D = SR.directions(S).astype(np.float64)
    u = D / np.sqrt((D * D).sum(axis=1))[:, None]
    k = rng.uniform(-0.3, 0.3, (3, 3))
    return base[None, :] + u @ k + 0.15 * (u[:, 1:2] ** 2)


def codes_of(S, rgb):
    t = np.ones((6 * S * S, 4), np.float16)
    t[:, :3] = np.asarray(rgb).astype(np.float16)
    return t.view(np.uint16).reshape(6, S, S, 4).copy()


def sun_cube(S, face, place, patch_degrees, smooth=True, level=4000.0, seed=0):
    """Background plus level (1 - angle / patch)^2 within `patch_degrees` of the direction through the peak texel's centre: the peak texel
    itself is the one at angle 0, the patch crosses the faces the place says."""
    x, y = peak_texel(S, place)
    i = (face * S + y) * S + x
    D = SR.directions(S).astype(np.float64)
    u = D / np.sqrt((D * D).sum(axis=1))[:, None]
    ang = np.degrees(np.arccos(np.clip(u @ u[i], -1.0, 1.0)))
    rgb = background(S, smooth, seed + 17 * face + S)
    sun = np.where(ang < patch_degrees, level * (1.0 - ang / patch_degrees) ** 2, 0.0)
    rgb = rgb + sun[:, None] * np.array([1.0, 0.9, 0.7])
    return codes_of(S, rgb), (face, x, y)


def placed(S, cone, ring, patch, faces=range(6), places=PLACES):
    out = []
    for face in faces:
        for place in places:
            codes, peak = sun_cube(S, face, place, patch, smooth=(face % 2 == 0))
            out.append(Case("S%d_face%d_%s" % (S, face, place), codes, cone, ring, faces=FACES_IN_CONE[place], peak=peak))
    return out


def plateau(S=16):
    """Four texels share the maximum, on two faces: the tie goes to the lowest index, (face 1, x 3, y 2)."""
    rgb = background(S, True, 5)
    codes = codes_of(S, rgb)
    for f, x, y in ((4, 8, 8), (1, 3, 2), (1, 4, 2), (1, 3, 3)):
        codes[f, y, x, :3] = np.array([3000.0, 3000.0, 3000.0], np.float16).view(np.uint16)
    return Case("plateau", codes, 20.0, 40.0, faces=None, peak=(1, 3, 2))


def hostile(S=16):
    """NaN, +inf, -inf, negatives and -0 inside the cone, in the ring and elsewhere; the peak itself is +inf in one channel (it reads 65504)."""
    codes, peak = sun_cube(S, 2, "edge", 12.0, smooth=True, seed=9)
    rng = np.random.default_rng(11)
    flat = codes.reshape(-1, 4)
    kind = rng.integers(0, 12, (flat.shape[0], 3))
    for k, code in ((0, 0x7E00), (1, 0xFC00), (2, 0xC500), (3, 0x8000), (4, 0xFE01)):      # NaN, -inf, -5, -0, another NaN
        flat[..., :3][kind == k] = code
    f, x, y = peak
    codes[f, y, x, :3] = (0x7C00, 0x7BFF, 0x7000)      # +inf, 65504, 8192
    return Case("hostile", codes, 20.0, 40.0, faces=2, peak=peak)


def constant(S=16, value=0.75):
    return Case("constant", codes_of(S, np.full((6 * S * S, 3), value)), 20.0, 40.0)


def black(S=16):
    return Case("black", codes_of(S, np.zeros((6 * S * S, 3))), 20.0, 40.0)


def degenerate():
    """Sides 1, 2, 3, 5 at 20 / 40 degrees: a cone of one texel (S = 1: the ring is empty, the background 0), an odd side.  Six or 24 texels
    hold no mean a peak could stand 16 times above: the contrast asked for is 2."""
    out = []
    for S in (1, 2, 3, 5):
        rng = np.random.default_rng(40 + S)
        rgb = rng.uniform(0.2, 1.5, (6 * S * S, 3))
        f, y, x = 3, S // 2, S - 1
        rgb[(f * S + y) * S + x] = (900.0, 800.0, 500.0)
        out.append(Case("S%d" % S, codes_of(S, rgb), 20.0, 40.0, 2.0, peak=(f, x, y)))
    return out


def gpu_cases():
    """S = 16 and 37 at 20 / 40 degrees -- every place on face 0, every face at its corner for 16, the three places on two faces for 37 (8214
    texels: nine chunks, no power of two) --, S = 64 with the default angles, the special cubes and the degenerate sides."""
    c = placed(16, 20.0, 40.0, 12.0, faces=(0,)) + placed(16, 20.0, 40.0, 12.0, faces=(1, 2, 3, 4, 5), places=("corner",))
    c += placed(37, 20.0, 40.0, 12.0, faces=(1, 2))
    c += placed(64, 0.0, 0.0, 3.0, faces=(5,), places=("centre", "corner"))
    return c + [plateau(), hostile(), constant(), black()] + degenerate()
