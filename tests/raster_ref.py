"""An exact model of the visibility pass: the contract in the header of oracle/orc_raster.h and the D3D11 rasterisation rules, restated
in exact arithmetic (Python integers and Fractions; numpy int64 only on snapped coordinates, whose bound |X|, |Y| < 2^30 keeps every
edge function below 2^63).  It is written from the contract, not from the kernels, and it is the judge of tests/raster_cases.py: coverage
and ownership are integer predicates on snapped coordinates, so there is exactly one right answer per pixel.

Per triangle: the clip-space vertices (exact rationals of fp32 values) -> near clip -> guard-band clip against x <= 256 w, x >= -256 w,
y <= 256 w, y >= -256 w in that order -> fan around the first vertex -> viewport transform, floor(v * 256 + 1/2) -> cull area2 <= 0 ->
candidate pixels whose centre lies in the box -> three edge functions, top-left rule -> z from the snapped barycentrics -> 0 <= z <= 1 ->
D24 = floor(z * (2^24 - 1) + 1/2) -> the smallest key (D24, ((inst << 24) | prim) + 1) wins against the cleared key (0xFFFFFF, 0): a
fragment at exactly z = 1 has code 0xFFFFFF and a word > 0, it loses (depth LESS against a buffer cleared to 1.0).

Where the model does not decide: the contract interpolates and snaps in fp32, the model exactly; tests/raster_cases.py only emits vertices
for which the two agree.  The vertex's z attribute is the fp32 nearest to z_clip / w_clip (the contract stores it as a float).  The
contract evaluates z0 + l1 dz1 + l2 dz2 in double: its error times 2^24 stays below 2^-27, so a winning fragment whose exact
z * (2^24 - 1) + 1/2 lies within 2^-20 of an integer is flagged "depth code ambiguous" and may legitimately round the other way; a
triangle of constant z is never flagged (dz1 = dz2 = 0: the double expression is z0 itself and z0 * (2^24 - 1) + 1/2 is exact in double).
A vertex with a NaN or infinite coordinate has no rational value: after the transform all four of its clip coordinates are NaN, it is
"behind" the near plane, every vertex the clipper derives from it is NaN and every fan triangle holds one of them, so the triangle is
dropped -- the model drops it at the door.
"""
from fractions import Fraction as Fr
import math

import numpy as np

GUARD = 256
D24_MAX = (1 << 24) - 1
CLEAR_DEPTH = 0xFFFFFF
AMBIGUOUS_LOG2 = 20


def fr32(x):
    """The exact value of an fp32 (or anything float() takes exactly)."""
    return Fr(float(x))


def round_f32(v):
    """The fp32 nearest to the rational v (ties to even), as a Fraction; normal range only."""
    if v == 0:
        return Fr(0)
    s, a = (-1 if v < 0 else 1), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fr(2) ** e > a:
        e -= 1
    e = max(e, -126)
    scale = Fr(2) ** (23 - e)
    n = a * scale
    q, r = divmod(n.numerator, n.denominator)
    if 2 * r > n.denominator or (2 * r == n.denominator and (q & 1)):
        q += 1
    return s * Fr(q) / scale


def clip_vertices(verts, wvp):
    """Exact clip-space positions: verts[n, >= 3] fp32 positions, wvp[4, 4] fp32 in the row-vector convention (clip_j = sum_i p_i M[i][j], p_3 = 1).
    Returns a list of 4-tuples of Fractions, or None for a vertex that is not finite."""
    M = [[fr32(wvp[i][j]) for j in range(4)] for i in range(4)]
    out, cache = [], {}
    for v in np.asarray(verts, np.float32)[:, :3]:
        k = v.tobytes()
        if k not in cache:
            if not np.all(np.isfinite(v)):
                cache[k] = None
            else:
                p = [fr32(v[0]), fr32(v[1]), fr32(v[2]), Fr(1)]
                cache[k] = tuple(sum(p[i] * M[i][j] for i in range(4)) for j in range(4))
        out.append(cache[k])
    return out


def _lerp(p, q, t):
    return tuple(a + (b - a) * t for a, b in zip(p, q))


def clip_near(tri):
    out = []
    for k in range(3):
        a, b = tri[k], tri[(k + 1) % 3]
        ia, ib = a[2] >= 0, b[2] >= 0
        if ia:
            out.append(a)
        if ia != ib:
            p, q = (a, b) if ia else (b, a)
            c = _lerp(p, q, p[2] / (p[2] - q[2]))
            out.append((c[0], c[1], Fr(0), c[3]))
    return out


def _guard_distance(v, plane):
    gw = GUARD * v[3]
    return (gw - v[0], gw + v[0], gw - v[1], gw + v[1])[plane]


def clip_guard(poly, plane):
    out, n = [], len(poly)
    for k in range(n):
        a, b = poly[k], poly[(k + 1) % n]
        da, db = _guard_distance(a, plane), _guard_distance(b, plane)
        ia, ib = da >= 0, db >= 0
        if ia:
            out.append(a)
        if ia != ib:
            (p, dp), (q, dq) = ((a, da), (b, db)) if ia else ((b, db), (a, da))
            c = list(_lerp(p, q, dp / (dp - dq)))
            gw = GUARD * c[3]
            c[plane >> 1] = gw if plane in (0, 2) else -gw
            out.append(tuple(c))
    return out


def clip_polygon(tri):
    """Near clip, then the guard band where a vertex leaves it: the polygon in clip space (possibly empty) and whether anything was clipped."""
    poly, clipped = list(tri), False
    if not all(v[2] >= 0 for v in tri):
        poly, clipped = clip_near(tri), True
    if any(abs(v[0]) > GUARD * v[3] or abs(v[1]) > GUARD * v[3] for v in poly):
        clipped = True
        for plane in range(4):
            poly = clip_guard(poly, plane)
    return poly, clipped


def snap(p, W, H):
    """Viewport transform and snapping of one clip-space vertex: (X, Y, z) or None (w <= 0, or beyond +-2^30)."""
    if not p[3] > 0:
        return None
    X = math.floor((p[0] / p[3] + 1) * Fr(W, 2) * 256 + Fr(1, 2))
    Y = math.floor((1 - p[1] / p[3]) * Fr(H, 2) * 256 + Fr(1, 2))
    if not (abs(X) < (1 << 30) and abs(Y) < (1 << 30)):
        return None
    return X, Y, round_f32(p[2] / p[3])


def _top_left(ax, ay, bx, by):
    # clockwise in y-down screen space is front: a top edge runs left -> right on a horizontal line, a left edge runs upwards
    dx, dy = bx - ax, by - ay
    return (dy == 0 and dx > 0) or dy < 0


class Result:
    """vis, depth: uint32 [H, W]; ambiguous, covered: bool [H, W]; count: how many fragments passed the depth clip on each pixel, sloped: how many
    of them came from a triangle whose z is not constant;
    polygons: per instance, {primitive: vertex count of its clipped polygon} for the triangles that were clipped;
    boxes: per instance, a list of (primitive, candidate pixels of the box inside the rows, clipped) per rasterised sub-triangle."""


def render(meshes, W, H, rows=None):
    """meshes: two (clip, idx) pairs, clip as clip_vertices() returns it, idx[n, 3].  The full frame is modelled (pixels are independent);
    `rows` only bounds the candidate boxes that Result.boxes reports."""
    r0, r1 = rows if rows else (0, H)
    best_d = np.full((H, W), CLEAR_DEPTH, np.int64)
    best_w = np.zeros((H, W), np.int64)
    amb = np.zeros((H, W), bool)
    count = np.zeros((H, W), np.int64)
    sloped = np.zeros((H, W), np.int64)
    seen = {}                    # identical snapped triangles (the later, higher word never wins): only their fragments are counted
    res = Result()
    res.polygons, res.boxes = [{}, {}], [[], []]
    snapped, prepared, masks = {}, {}, {}
    for inst, (clip, idx) in enumerate(meshes):
        for prim, tri in enumerate(np.asarray(idx).reshape(-1, 3).tolist()):
            cv = [clip[i] for i in tri]
            if any(c is None for c in cv):
                continue
            key = (id(cv[0]), id(cv[1]), id(cv[2]))          # (clip_vertices hands out one object per distinct vertex)
            if key not in prepared:
                poly, clipped = clip_polygon(cv)
                subs = []
                for sub in range(len(poly) - 2):
                    sv = []
                    for p in (poly[0], poly[sub + 1], poly[sub + 2]):
                        if p not in snapped:
                            snapped[p] = snap(p, W, H)
                        sv.append(snapped[p])
                    if all(s is not None for s in sv):
                        subs.append(sv)
                prepared[key] = (len(poly), clipped, subs)
            npoly, clipped, subs = prepared[key]
            if clipped:
                res.polygons[inst][prim] = npoly
            word = ((inst << 24) | prim) + 1
            for sv in subs:
                (X0, Y0, z0), (X1, Y1, z1), (X2, Y2, z2) = sv
                area2 = (X1 - X0) * (Y2 - Y0) - (Y1 - Y0) * (X2 - X0)
                if area2 <= 0:
                    continue
                # pixel px is a candidate when its centre px * 256 + 128 lies in [min, max]
                px0, px1 = -((128 - min(X0, X1, X2)) // 256), (max(X0, X1, X2) - 128) // 256
                py0, py1 = -((128 - min(Y0, Y1, Y2)) // 256), (max(Y0, Y1, Y2) - 128) // 256
                px0, py0, px1, py1 = max(px0, 0), max(py0, 0), min(px1, W - 1), min(py1, H - 1)
                if px0 > px1 or py0 > py1:
                    continue
                sy0, sy1 = max(py0, r0), min(py1, r1 - 1)
                if sy0 <= sy1:
                    res.boxes[inst].append((prim, (px1 - px0 + 1) * (sy1 - sy0 + 1), clipped))
                geometry = (inst, X0, Y0, X1, Y1, X2, Y2, z0, z1, z2)
                if geometry in seen:
                    if seen[geometry] is not None:
                        count[py0:py1 + 1, px0:px1 + 1] += seen[geometry]
                    continue
                seen[geometry] = None
                shape = geometry[1:7]
                if z0 == z1 == z2 and shape in masks:            # (the same snapped triangle at another constant depth: its coverage is known)
                    inside = masks[shape]
                else:
                    PX = (np.arange(px0, px1 + 1, dtype=np.int64) * 256 + 128)[None, :]
                    PY = (np.arange(py0, py1 + 1, dtype=np.int64) * 256 + 128)[:, None]
                    w0 = (X2 - X1) * (PY - Y1) - (Y2 - Y1) * (PX - X1)
                    w1 = (X0 - X2) * (PY - Y2) - (Y0 - Y2) * (PX - X2)
                    w2 = (X1 - X0) * (PY - Y0) - (Y1 - Y0) * (PX - X0)
                    inside = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
                    if not _top_left(X1, Y1, X2, Y2):
                        inside &= w0 != 0
                    if not _top_left(X2, Y2, X0, Y0):
                        inside &= w1 != 0
                    if not _top_left(X0, Y0, X1, Y1):
                        inside &= w2 != 0
                    masks[shape] = inside
                if not inside.any():
                    continue
                bd, bw, ba, bc = (a[py0:py1 + 1, px0:px1 + 1] for a in (best_d, best_w, amb, count))
                if z0 == z1 == z2:
                    if not 0 <= z0 <= 1:
                        continue
                    d = np.full(inside.shape, math.floor(z0 * D24_MAX + Fr(1, 2)), np.int64)
                    a = np.zeros(inside.shape, bool)
                else:
                    # z * (2^24 - 1) + 1/2 = num / den with Python integers (object arrays): z_k = n_k / 2^E
                    E = max(z.denominator for z in (z0, z1, z2))
                    n0, n1, n2 = (int(z * E) for z in (z0, z1, z2))
                    ys, xs = np.nonzero(inside)
                    u1, u2 = w1[ys, xs].astype(object), w2[ys, xs].astype(object)
                    zn = area2 * n0 + u1 * (n1 - n0) + u2 * (n2 - n0)          # z = zn / (area2 * E)
                    zd = area2 * E
                    ok = np.array([0 <= v <= zd for v in zn], bool)
                    num, den = zn * (2 * D24_MAX) + zd, 2 * zd
                    q = np.array([v // den for v in num], np.int64)
                    rem = np.array([v % den for v in num], object)
                    near = np.array([min(v, den - v) << AMBIGUOUS_LOG2 <= den for v in rem], bool)
                    inside = np.zeros(inside.shape, bool)
                    inside[ys[ok], xs[ok]] = True
                    d = np.zeros(inside.shape, np.int64)
                    a = np.zeros(inside.shape, bool)
                    d[ys, xs] = q
                    a[ys, xs] = near
                bc += inside
                if z0 == z1 == z2:
                    seen[geometry] = inside
                else:
                    sloped[py0:py1 + 1, px0:px1 + 1] += inside
                win = inside & ((d < bd) | ((d == bd) & (word < bw)))
                bd[win], bw[win], ba[win] = d[win], word, a[win]
    res.vis, res.depth = best_w.astype(np.uint32), best_d.astype(np.uint32)
    res.ambiguous, res.covered, res.count, res.sloped = amb, best_w != 0, count, sloped
    return res
