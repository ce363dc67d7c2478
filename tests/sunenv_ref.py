"""The sun from the environment restated with numpy from the contract in include/rtggx.h (rtggx_sun_from_env) and not from the kernels:
the texel rule, the integer directions and masks, the weights, every sum in the contract's pairwise order (score_ref.tree_sum), the host's
arithmetic, the cut level 0 and -- through envimage_ref's chain -- the cube the removal leaves.  numpy's float64 arithmetic is the same
IEEE arithmetic, one rounding per ufunc; what a device might differ by is a double sqrt or divide that is an ulp off (DERIVED_BOUND);
gfx950 does not (DEVICE_BOUND).

A level 0 is RGBA16F codes, uint16 [6, S, S, 4] (env_cases.Cube.codes[0]); texel (f, x, y) has the index i = (f S + y) S + x."""
import numpy as np

import envimage_ref as E
from score_ref import tree_sum

DEFAULT_CONE, DEFAULT_RING_FACTOR, DEFAULT_CONTRAST = 4.0, 3.0, 16.0
MAX_SIDE = 8192
# DERIVED_BOUND: |a sum - the same sum evaluated otherwise| <= DERIVED_BOUND x sum |terms|.  A term is at most 8 roundings from its exact
# inputs (n q, the quotient w, the product with Y or v -- Y(e) itself is exact --, D / q, the product with d, and a sqrt and two divides that
# might each be one ulp, not half, off), each 2^-53 relative, and the pairwise tree adds at most ceil(log2(6 x 8192^2)) = 29 < 32 levels
# of 2^-53 each: 8 + 32 = 40 < 64.  It is what holds between two ORDERS of one sum (the host tests), and what a device whose double sqrt or
# divide were an ulp off would have to meet.
# DEVICE_BOUND, the bound in force between the device and this model: 0.  Measured on gfx950 over every case of tests/sunenv_cases.py, every
# sum of the device was the model's to the last bit -- its fp64 sqrt and divide round correctly, the terms are the model's and the tree is
# the same tree --, so the derived bound was tightened to equality of the values (a zero may carry either sign).
DERIVED_BOUND = 64.0 * 2.0 ** -53
DEVICE_BOUND = 0.0
SUMS = ("weight_all", "weight_cone", "weight_ring", "ring_rgb", "excess", "moment")


def values(codes):
    """uint16 [6, S, S, 4] -> float64 [6 S^2, 3]: per channel x > 0 ? min(x, 65504) : 0."""
    x = np.ascontiguousarray(codes)[..., :3].copy().view(np.float16).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.minimum(x, 65504.0), 0.0)


def luma(c):
    return (0.25 * c[..., 0] + 0.5 * c[..., 1]) + 0.25 * c[..., 2]


def directions(S):
    """int64 [6 S^2, 3]: D = S cubeFaceDir(f, a / S, b / S), a = 2 x + 1 - S, b = 2 y + 1 - S."""
    f, y, x = np.meshgrid(np.arange(6), np.arange(S), np.arange(S), indexing="ij")
    f, a, b = f.reshape(-1), (2 * x + 1 - S).reshape(-1), (2 * y + 1 - S).reshape(-1)
    s = np.full_like(a, S)
    table = ((s, -b, -a), (-s, -b, a), (a, s, b), (a, -s, -b), (a, -b, s), (-a, -b, -s))
    D = np.zeros((6 * S * S, 3), np.int64)
    for face, d in enumerate(table):
        k = f == face
        for c in range(3):
            D[k, c] = d[c][k]
    return D


def cos2(degrees):
    c = np.cos(np.float64(np.float32(degrees)) * (3.14159265358979323846 / 180.0))
    return float(c * c)


def angles(cone=0.0, ring=0.0, min_contrast=0.0):
    """The arguments with 0 replaced by the defaults, as float32 values."""
    cone = np.float32(cone) if cone else np.float32(DEFAULT_CONE)
    ring = np.float32(ring) if ring else np.float32(DEFAULT_RING_FACTOR) * cone
    return cone, ring, (np.float32(min_contrast) if min_contrast else np.float32(DEFAULT_CONTRAST))


def masks(S, peak_index, cos2_cone, cos2_ring):
    """(cone, ring) bool [6 S^2] about texel `peak_index`: dot > 0 and dot dot >= (cos2 n) nP, in float64, each product rounded on its own."""
    D = directions(S)
    P = D[peak_index]
    dot = (D @ P).astype(np.float64)      # integers below 2^53: exact
    n, nP = (D * D).sum(axis=1).astype(np.float64), np.float64((P * P).sum())
    cone = (dot > 0) & (dot * dot >= (np.float64(cos2_cone) * n) * nP)
    ring = ~cone & (dot > 0) & (dot * dot >= (np.float64(cos2_ring) * n) * nP)
    return cone, ring


def half_of(background):
    """float64 [3] -> (binary16 codes uint16 [3], the same as float32 [3]): (float)background capped at 65504, rounded to nearest even."""
    f = np.minimum(np.asarray(background, np.float64).astype(np.float32), np.float32(65504.0))
    h = np.where(f > 0, f, np.float32(0.0)).astype(np.float16)
    return h.view(np.uint16), h.astype(np.float32)


def host_result(moment, excess, weight_all):
    """(found, direction float32 [3], irradiance float32 [3]) from the three sums, as the host derives them."""
    m = np.asarray(moment, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    if not np.isfinite(length) or not length > 0.0:
        return 0, np.zeros(3, np.float32), np.zeros(3, np.float32)
    scale = 4.0 * 3.14159265358979323846 / np.float64(weight_all)
    return 1, (m / length).astype(np.float32), (np.asarray(excess, np.float64) * scale).astype(np.float32)


def estimate(codes, cone=0.0, ring=0.0, min_contrast=0.0, remove=False, given=None):
    """The record rtggx_sun_from_env must return for level 0 `codes`, as a dict with capi.SunEstimate's names, plus "sum_wy" (the sum behind
    mean_luma), "magnitude": per sum the sum of |terms| (what the bounds multiply), "cone_mask" / "ring_mask" and "b16_codes".  given: a
    device record (or a part of one) whose cos2_cone, cos2_ring and background_half are taken over instead of computed, for the comparisons
    that must then be bit for bit."""
    codes = np.ascontiguousarray(codes, np.uint16)
    S = codes.shape[1]
    assert codes.shape == (6, S, S, 4) and S <= MAX_SIDE
    cone_deg, ring_deg, contrast = angles(cone, ring, min_contrast)
    v = values(codes)
    Y = luma(v)
    peak = int(np.argmax(Y))      # (the first of equal maxima: the lowest index)
    given = given or {}
    r = {"cos2_cone": float(given.get("cos2_cone", cos2(cone_deg))), "cos2_ring": float(given.get("cos2_ring", cos2(ring_deg))),
         "peak_luma": float(Y[peak]), "peak_face": peak // (S * S), "peak_y": (peak % (S * S)) // S, "peak_x": peak % S}
    in_cone, in_ring = masks(S, peak, r["cos2_cone"], r["cos2_ring"])
    D = directions(S).astype(np.float64)
    n = (D * D).sum(axis=1)
    q = np.sqrt(n)
    w = (4.0 * S) / (n * q)
    d = D / q[:, None]
    zero = np.zeros_like(w)
    mag = {}

    def total(name, terms):
        mag[name] = np.abs(terms).sum(axis=0)
        return tree_sum(terms) if terms.ndim == 1 else np.array([tree_sum(terms[:, c]) for c in range(terms.shape[1])])

    r["weight_all"] = total("weight_all", w)
    sum_wy = total("sum_wy", w * Y)
    r["weight_ring"] = total("weight_ring", np.where(in_ring, w, zero))
    r["ring_rgb"] = total("ring_rgb", np.where(in_ring[:, None], w[:, None] * v, 0.0))
    r["texels_cone"], r["texels_ring"] = int(in_cone.sum()), int(in_ring.sum())
    r["sum_wy"], r["mean_luma"] = sum_wy, float(sum_wy / r["weight_all"])
    r["background"] = r["ring_rgb"] / r["weight_ring"] if r["weight_ring"] > 0.0 else np.zeros(3)
    if "background_half" not in given:
        b16_codes, b16 = half_of(r["background"])
    else:
        b16 = np.asarray(given["background_half"], np.float32)
        b16_codes = b16.astype(np.float16).view(np.uint16)
        assert (b16_codes.view(np.float16).astype(np.float32) == b16).all()
    r["background_half"], r["b16_codes"] = b16, b16_codes
    r["found"] = 0 if (r["peak_luma"] == 0.0 or r["peak_luma"] < np.float64(contrast) * r["mean_luma"]) else 1
    r["weight_cone"], r["excess"], r["moment"], r["texels_lit"] = 0.0, np.zeros(3), np.zeros(3), 0
    r["direction"], r["irradiance"], r["removed"] = np.zeros(3, np.float32), np.zeros(3, np.float32), 0
    if r["found"]:
        e = np.where(in_cone[:, None], np.maximum(v - b16.astype(np.float64), 0.0), 0.0)
        r["weight_cone"] = total("weight_cone", np.where(in_cone, w, zero))
        r["excess"] = total("excess", w[:, None] * e)
        r["moment"] = total("moment", (w * luma(e))[:, None] * d)
        r["texels_lit"] = int((e > 0).any(axis=1).sum())
        r["found"], r["direction"], r["irradiance"] = host_result(r["moment"], r["excess"], r["weight_all"])
    r["removed"] = 1 if (remove and r["found"]) else 0
    r["magnitude"], r["cone_mask"], r["ring_mask"] = mag, in_cone, in_ring
    return r


def split(codes, rec):
    """(residual, e) float64 [6 S^2, 3] of the SANITISED texel values: in the cone min(v, b16) and max(v - b16, 0), elsewhere v and 0."""
    v = values(codes)
    b = np.asarray(rec["background_half"], np.float64)
    cone = rec["cone_mask"][:, None]
    return np.where(cone, np.minimum(v, b), v), np.where(cone, np.maximum(v - b, 0.0), 0.0)


def removed_level0(codes, rec):
    """Level 0 after the removal: at the cone's texels r, g, b = min(v, b16) as binary16 codes, alpha kept; every other texel bit for bit."""
    codes = np.ascontiguousarray(codes, np.uint16)
    out = codes.copy().reshape(-1, 4)
    cut = np.minimum(values(codes), np.asarray(rec["background_half"], np.float64)).astype(np.float16).view(np.uint16)
    k = rec["cone_mask"]
    out[k, :3] = cut[k]
    return out.reshape(codes.shape)


def cube_of(level0_codes):
    """RTGGX_BUF_ENV of a level 0 and the full box chain below it (rtggx_generate_env_mips' rule): uint16 [texels, 4], mip-major."""
    level0_codes = np.ascontiguousarray(level0_codes, np.uint16)
    levels = E.chain(level0_codes[..., :3].copy().view(np.float16).astype(np.float32))
    return np.concatenate([level0_codes.reshape(-1, 4), E.pack(levels[1:])]) if len(levels) > 1 else level0_codes.reshape(-1, 4)


def chain_codes(level0_codes):
    """The same cube as env_cases.Cube wants it: per level the codes uint16 [6, s, s, 4]."""
    buf, out, at = cube_of(level0_codes), [], 0
    for s in E.chain_sides(level0_codes.shape[1]):
        out.append(buf[at:at + 6 * s * s].reshape(6, s, s, 4).copy()); at += 6 * s * s
    return out
