"""Synthetic triangles for the software rasteriser, built so that the exact model (tests/raster_ref.py) is the only right answer.

The contract (oracle/orc_raster.h) transforms, clips and snaps in fp32; the model does it exactly.  The model can only be the judge where
the two agree, so check_robust() evaluates the contract's fp32 chain for every triangle of every case in numpy.float32 -- once with separate
multiplies and adds, once with every a * b + c fused (the device contracts, the oracle is built with -ffp-contract=off) -- and the exact
chain, and raises unless all three give the same polygon, the same snapped integers and the same fp32 z.  How the cases get there:
positions are X / (128 W) - 1 for integer sub-pixel X (a quarter unit added where asked for; half units, the snapping ties, only at
power-of-two frame sizes where the chain is exact), clip-space values of the clipped triangles are dyadic (t = 1/2 on every cut edge).

Depth: overlapping triangles have constant z each (their depth code is exact); a sloped triangle overlaps nothing (check(),
with the model: every pixel a sloped fragment lands on holds exactly one fragment), its depths are drawn from values such as 0.3 and
0.7, and the model's "ambiguous" flag may exempt at most 1 % of a case's covered pixels from the depth comparison (none from visibility).

Families (the numbers of the issue that asked for them are kept as prefixes of the case names):
  1 fill rule, 2 watertight meshes, 3 small/large threshold, 4 wave work sharing, 5 depth resolve, 6 clipping, 7 frames and strips,
  8 full large-triangle queue, 9 tile words.
"""
from fractions import Fraction as Fr
import math

import numpy as np

import raster_ref as R

SMALL_BOX = 1024          # visibility.hip RT_SMALL_BOX: a box of more candidate pixels goes to the tile pass
LARGE_CAPACITY = 65536    # the large-triangle queue
IDENTITY = np.eye(4, dtype=np.float32)
AMBIGUOUS_CAP = 0.01
APRON = 18                # the visibility pass draws the strip's rows and 18 more on each side (rtggx_context.h passRows, ROWS_GBUFFER)


def kernel_rows(strip, H):
    """The rows the rasterisers get for a strip: their rowBegin and rowEnd.  Boxes are clamped to these, rasterLarge's blocks and the tile words
    are counted from the first of them, and every one of them is drawn, so the tests compare all of them."""
    return max(strip[0] - APRON, 0), min(strip[1] + APRON, H)


def perspective(a, b):
    """clip = (x, y, a z + b, z): w is the input's z, depth is a + b / z."""
    m = np.zeros((4, 4), np.float32)
    m[0][0] = m[1][1] = 1.0
    m[2][2], m[3][2], m[2][3] = a, b, 1.0
    return m


class Case:
    def __init__(self, name, W, H, strips=None, wvp=(IDENTITY, IDENTITY)):
        self.name, self.W, self.H = name, W, H
        self.strips = strips or [(0, H)]
        self.wvp = [np.asarray(m, np.float32) for m in wvp]
        self.v = [[], []]
        self.i = [[], []]
        self.polygons = {}          # (inst, prim) -> expected vertex count of the clipped polygon
        self.once = False           # every pixel of the frame holds exactly one fragment
        self.lanes = None           # {lane index in the triangle list: expected candidate count} (family 4)
        self.wave_totals = None     # {wave: expected total}
        self.drawn = None           # expected number of covered pixels, where the case knows it
        self.expect = []            # (x, y, word or None, depth code or None): known answers
        self.large_at_least = 0     # so many triangles go to the tile pass
        self.clipped = 0            # so many triangles are clipped (near plane or guard band): check_robust counts them
        self.once_at = []           # (x, y): pixels that hold exactly one fragment, and are drawn
        self.winners = None         # (lo, hi, at least) over the concatenated triangle list
        self.levels = None          # perspective cases: the w values a triangle's z selects (see tri())
        self.strip_lanes = None     # {strip: {lane: expected candidate count inside the rows the kernels get for it}}
        self.tile_strips = []       # strips for which the tile of some drawn pixel depends on the pass's first row
        self._model = None

    # ---- building
    def ndc(self, X, Y):
        """Sub-pixel coordinates (units of 1/256 pixel; multiples of 1/4 allowed) to fp32 NDC."""
        return np.float32(Fr(X) / (128 * self.W) - 1), np.float32(1 - Fr(Y) / (128 * self.H))

    def raw(self, inst, a, b, c):
        """A triangle of three (x, y, z) positions as they go into the vertex buffer."""
        base = len(self.v[inst])
        self.v[inst] += [tuple(np.float32(t) for t in p) for p in (a, b, c)]
        self.i[inst].append((base, base + 1, base + 2))
        return len(self.i[inst]) - 1

    def tri(self, inst, a, b, c, front=True):
        """A triangle of three (X, Y, z) in sub-pixel units, wound clockwise on the y-down screen (front) or the other way round."""
        area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if (area2 > 0) != front and area2 != 0:
            b, c = c, b
        if self.levels:
            # under perspective(a, b) a triangle lies at one w = z_in (a power of two, so x w and y w are exact): its depth is a + b / w
            w = self.levels[int(round(a[2] * 128)) % len(self.levels)]
            return self.raw(inst, *[(self.ndc(p[0], p[1])[0] * np.float32(w), self.ndc(p[0], p[1])[1] * np.float32(w), w) for p in (a, b, c)])
        return self.raw(inst, *[(*self.ndc(p[0], p[1]), p[2]) for p in (a, b, c)])

    def rect(self, inst, x0, y0, x1, y1, z):
        """Pixels [x0, x1) x [y0, y1) as two triangles whose boxes both hold (x1 - x0) * (y1 - y0) candidates."""
        a, b, c, d = (x0 * 256, y0 * 256, z), (x1 * 256, y0 * 256, z), (x1 * 256, y1 * 256, z), (x0 * 256, y1 * 256, z)
        return self.tri(inst, a, b, c), self.tri(inst, a, c, d)

    def corner(self, inst, x, y, w, h, z):
        """A right triangle with its corner on pixel corner (x, y): a box of exactly w * h candidates."""
        return self.tri(inst, (x * 256, y * 256, z), ((x + w) * 256, y * 256, z), (x * 256, (y + h) * 256, z))

    def dot(self, inst, x, y, z):
        """A triangle that covers the centre of pixel (x, y) and nothing else: one candidate."""
        return self.tri(inst, (x * 256 + 16, y * 256 + 16, z), (x * 256 + 250, y * 256 + 16, z), (x * 256 + 16, y * 256 + 250, z))

    def filler(self):
        """Both mesh slots hold real triangles: a slot the case left empty gets one dot at the far plane's side."""
        for inst in range(2):
            if not self.i[inst]:
                self.dot(inst, 0, 0, 0.96875)
        return self

    # ---- what the tests use
    def mesh(self, inst):
        v = np.zeros((len(self.v[inst]), 6), np.float32)
        v[:, :3] = np.asarray(self.v[inst], np.float32).reshape(-1, 3)
        v[:, 5] = -1.0
        return v, np.asarray(self.i[inst], np.uint32).reshape(-1)

    def constants(self):
        fc = np.zeros(768, np.uint8)
        f = fc.view(np.float32)
        for inst in range(2):
            t = self.wvp[inst].T.reshape(-1)       # stored transposed: M[i][j] = f[j * 4 + i]
            f[16 * inst:16 * inst + 16] = t         # WorldViewProjs
            f[32 + 16 * inst:48 + 16 * inst] = t    # WorldViewProjsPrev
            f[136 + 20 * inst:152 + 20 * inst] = t  # perObject[inst].WorldViewProj (byte 544 + 80 inst); ProjBias stays 0
        return fc

    def model(self):
        if self._model is None:
            self._model = R.render(self.model_meshes(), self.W, self.H)
        return self._model

    def lane_counts(self, rows=None):
        """Candidate pixels per triangle of the concatenated list as rasterSmall's phase 2 sees them inside `rows`: 0 for a triangle that is
        culled, clipped (tile pass) or larger than the threshold."""
        m = self.model() if rows is None or tuple(rows) == (0, self.H) else R.render(self.model_meshes(), self.W, self.H, rows)
        n0 = len(self.i[0])
        out = np.zeros(n0 + len(self.i[1]), np.int64)
        for inst in range(2):
            for prim, cnt, clipped in m.boxes[inst]:
                if not clipped and cnt <= SMALL_BOX:
                    out[inst * n0 + prim] = cnt
        return out

    def model_meshes(self):
        return [(R.clip_vertices(np.asarray(self.v[k], np.float32).reshape(-1, 3), self.wvp[k]), np.asarray(self.i[k]).reshape(-1, 3)) for k in range(2)]

    def large_count(self):
        m = self.model()
        return sum(1 for inst in range(2) for _, cnt, clipped in m.boxes[inst] if clipped or cnt > SMALL_BOX)


# ---- the contract's fp32 chain, for check_robust ---------------------------------------------------------------------------------------
class F32:
    """fp32 arithmetic; muladd(a, b, c) = a * b + c rounds once (fused) or twice."""

    def __init__(self, fused):
        self.fused = fused

    def muladd(self, a, b, c):
        if self.fused:
            p, c64 = float(a) * float(b), float(c)          # the product of two fp32 is exact in double
            t = p + c64
            if not math.isfinite(t) or (t - p) - c64 == 0.0 and (t - (t - p)) - p == 0.0:      # the sum too (two-sum): one rounding is left
                return np.float32(t)
            return np.float32(float(R.round_f32(R.fr32(a) * R.fr32(b) + R.fr32(c))))
        return np.float32(np.float32(a * b) + c)


def _chain32(A, pos, M, W, H):
    """One triangle through the contract in fp32: the list of (X, Y, z) of its polygon (None for a vertex that is not snapped), in order."""
    f = np.float32
    one, half = f(1), f(0.5)
    cp = []
    for p in pos:
        c = []
        for j in range(4):
            t = f(p[0] * M[0][j])
            t = A.muladd(p[1], M[1][j], t)
            t = A.muladd(p[2], M[2][j], t)
            c.append(f(t + M[3][j]))
        cp.append(c)

    def lerp(p, q, t, comps):
        return [A.muladd(f(q[k] - p[k]), t, p[k]) if k in comps else None for k in range(4)]

    poly = cp
    if not all(c[2] >= 0 for c in cp):
        poly = []
        for k in range(3):
            a, b = cp[k], cp[(k + 1) % 3]
            ia, ib = a[2] >= 0, b[2] >= 0
            if ia:
                poly.append(a)
            if ia != ib:
                p, q = (a, b) if ia else (b, a)
                c = lerp(p, q, f(p[2] / f(p[2] - q[2])), (0, 1, 3))
                c[2] = f(0)
                poly.append(c)

    def dist(v, plane):
        g, s = f(256), (f(-1), f(1))[plane & 1]
        return A.muladd(g, v[3], f(s * v[plane >> 1]))

    if any(abs(v[0]) > f(f(256) * v[3]) or abs(v[1]) > f(f(256) * v[3]) for v in poly):
        for plane in range(4):
            out, n = [], len(poly)
            for k in range(n):
                a, b = poly[k], poly[(k + 1) % n]
                da, db = dist(a, plane), dist(b, plane)
                ia, ib = da >= 0, db >= 0
                if ia:
                    out.append(a)
                if ia != ib:
                    (p, dp), (q, dq) = ((a, da), (b, db)) if ia else ((b, db), (a, da))
                    c = lerp(p, q, f(dp / f(dp - dq)), (0, 1, 2, 3))
                    gw = f(f(256) * c[3])
                    c[plane >> 1] = gw if plane in (0, 2) else f(-gw)
                    out.append(c)
            poly = out
    res = []
    for p in poly:
        if not p[3] > 0:
            res.append(None)
            continue
        nx, ny = f(p[0] / p[3]), f(p[1] / p[3])
        sx, sy = f(f(nx + one) * f(f(W) * half)), f(f(one - ny) * f(f(H) * half))
        fx, fy = math.floor(A.muladd(sx, f(256), half)), math.floor(A.muladd(sy, f(256), half))
        res.append(None if not (abs(fx) < 2 ** 30 and abs(fy) < 2 ** 30) else (fx, fy, R.fr32(f(p[2] / p[3]))))
    return res


_ROBUST = {}


def check_robust(case):
    """Raises unless the fp32 chain (separate and fused) and the exact chain agree on every triangle of the case: the same polygon, the same
    snapped integers, the same fp32 z.  An unclipped triangle is checked vertex by vertex (a vertex is transformed and snapped on its own), a
    clipped one whole.  Returns (vertices, clipped triangles) of the case that went through the check, now or for an earlier case with the same
    transform and frame; the second must be the number the case states (Case.clipped)."""
    vertices = clipped_tris = 0
    with np.errstate(all="ignore"):
        for inst in range(2):
            M = case.wvp[inst]
            done = _ROBUST.setdefault((M.tobytes(), case.W, case.H), {"tri": {}, "vertex": set()})
            verts = np.asarray(case.v[inst], np.float32).reshape(-1, 3)
            for tri in case.i[inst]:
                pos = verts[list(tri)]
                if not np.all(np.isfinite(pos)):
                    continue                                  # dropped by contract and model alike (raster_ref.py)
                tkey = pos.tobytes()
                if tkey not in done["tri"]:
                    poly, clipped = R.clip_polygon(R.clip_vertices(pos, M))
                    if clipped:
                        _agree(case, inst, pos, M, [R.snap(p, case.W, case.H) for p in poly])
                    done["tri"][tkey] = clipped
                if done["tri"][tkey]:
                    clipped_tris += 1
                    continue
                for p in pos:
                    vertices += 1
                    if p.tobytes() not in done["vertex"]:
                        u = np.repeat(p[None], 3, 0)
                        _agree(case, inst, u, M, [R.snap(q, case.W, case.H) for q in R.clip_vertices(u, M)])
                        done["vertex"].add(p.tobytes())
    assert clipped_tris == case.clipped, "%s: %d clipped triangles went through the check, built for %d" % (case.name, clipped_tris, case.clipped)
    return vertices, clipped_tris


def _agree(case, inst, u, M, exact):
    for fused in (False, True):
        got = _chain32(F32(fused), u, M, case.W, case.H)
        if got != exact:
            raise AssertionError("%s: instance %d triangle %s is not robust (%s): fp32 %s, exact %s" %
                                 (case.name, inst, u.tolist(), "fused" if fused else "separate", got, exact))


def check(case):
    """The case's own conditions, checked with the model; returns the model's result."""
    m = case.model()
    covered = int(m.covered.sum())
    assert all(len(case.i[k]) > 0 for k in range(2)), "%s: both mesh slots hold triangles" % case.name
    assert not ((m.sloped > 0) & (m.count != 1)).any(), "%s: a sloped triangle overlaps another fragment" % case.name
    assert int(m.ambiguous.sum()) <= AMBIGUOUS_CAP * covered, "%s: %d of %d covered pixels have an ambiguous depth code" % (case.name, m.ambiguous.sum(), covered)
    for key, n in case.polygons.items():
        assert m.polygons[key[0]].get(key[1], 3) == n, "%s: triangle %s clipped to %s vertices, built for %d" % (case.name, key, m.polygons[key[0]].get(key[1]), n)
    for x, y in case.once_at:
        assert m.count[y, x] == 1 and m.covered[y, x], "%s: pixel (%d, %d) holds %d fragments, built for one" % (case.name, x, y, m.count[y, x])
    if case.once:
        assert (m.count == 1).all(), "%s: %d pixels are not covered exactly once" % (case.name, (m.count != 1).sum())
    if case.drawn is not None:
        assert covered == case.drawn, "%s: %d pixels covered, built for %d" % (case.name, covered, case.drawn)
    for x, y, word, depth in case.expect:
        assert word is None or m.vis[y, x] == word, "%s: pixel (%d, %d) word %#x, built for %#x" % (case.name, x, y, m.vis[y, x], word)
        assert depth is None or m.depth[y, x] == depth, "%s: pixel (%d, %d) depth %#x, built for %#x" % (case.name, x, y, m.depth[y, x], depth)
    if case.lanes or case.wave_totals:
        cnt = case.lane_counts()
        for lane, n in (case.lanes or {}).items():
            assert cnt[lane] == n, "%s: triangle %d has %d candidates, built for %d" % (case.name, lane, cnt[lane], n)
        for wave, n in (case.wave_totals or {}).items():
            assert cnt[64 * wave:64 * wave + 64].sum() == n, "%s: wave %d has %d candidates, built for %d" % (case.name, wave, cnt[64 * wave:64 * wave + 64].sum(), n)
    assert case.large_count() >= case.large_at_least, "%s: %d triangles for the tile pass, built for %d" % (case.name, case.large_count(), case.large_at_least)
    for strip, lanes in (case.strip_lanes or {}).items():
        rows = kernel_rows(strip, case.H)
        assert strip in case.strips and rows != (0, case.H), "%s: strip %s gives the kernels the whole frame" % (case.name, strip)
        cnt = case.lane_counts(rows)
        for lane, n in lanes.items():
            assert cnt[lane] == n, "%s: triangle %d has %d candidates in rows %s, built for %d" % (case.name, lane, cnt[lane], rows, n)
    for strip in case.tile_strips:
        # a tile index that forgets the pass's first row must mark other tiles: some drawn pixel INSIDE the strip lies in a tile that no drawn
        # pixel of the pass's rows would mark that way
        rb, re = kernel_rows(strip, case.H)
        assert strip in case.strips and rb % 16 != 0
        tx = (case.W + 15) // 16
        ys, xs = np.nonzero(m.covered[rb:re]); ys += rb
        wrong = set(((ys >> 4) * tx + (xs >> 4)).tolist())
        inside = (ys >= strip[0]) & (ys < strip[1])
        right = set((((ys - rb) >> 4) * tx + (xs >> 4))[inside].tolist())
        assert len(right - wrong) >= 2, "%s: strip %s has no drawn tile that only the right index marks" % (case.name, strip)
    if case.winners:
        n0 = len(case.i[0])
        words = np.unique(m.vis[m.covered]).astype(np.int64) - 1
        index = (words >> 24) * n0 + (words & 0xFFFFFF)
        for lo, hi, least in case.winners:
            got = int(((index >= lo) & (index < hi)).sum())
            assert got >= least, "%s: %d distinct winners among triangles %d..%d, built for at least %d" % (case.name, got, lo, hi, least)
    return m


# ---- what both test files do with a case -------------------------------------------------------------------------------------------------
def oracle_frame(c):
    """The CPU oracle's visibility and depth words for the case's full frame, computed once per case and kept."""
    if getattr(c, "_oracle", None) is None:
        from oracle import oracle as O
        o = O.Oracle(c.W, c.H, threads=1)
        try:
            for slot in range(2):
                o.set_mesh(slot, *c.mesh(slot))
            o.set_frame_constants(c.constants().tobytes())
            o.render_visibility()
            c._oracle = (o.buffer(O.BUF_VISIBILITY).reshape(c.H, c.W).copy(), o.buffer(O.BUF_DEPTH).reshape(c.H, c.W).copy())
        finally:
            o.close()
    return c._oracle


def compare(label, vis, depth, m, rows):
    """`vis`, `depth` [H, W] against the model inside `rows`: no pixel is exempt for visibility, only the model's flagged pixels for depth, and
    those by one code at the most."""
    s = slice(*rows)
    bad = vis[s] != m.vis[s]
    assert not bad.any(), "%s: %d visibility words differ from the model, first at (x, y) = %s" % (label, bad.sum(), np.argwhere(bad)[0][::-1] + (0, rows[0]))
    d = np.abs(depth[s].astype(np.int64) - m.depth[s].astype(np.int64))
    firm = d * ~m.ambiguous[s]
    assert not firm.any(), "%s: %d depth codes differ from the model, first at (x, y) = %s" % (label, (firm != 0).sum(), np.argwhere(firm)[0][::-1] + (0, rows[0]))
    assert not (d > 1).any(), "%s: a flagged depth code is off by %d" % (label, d.max())


# ---- family 1: fill rule -------------------------------------------------------------------------------------------------------------------
DIRS8 = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


def fill_rule_cases():
    out = []
    # the quad of test_oracle_known_answers.py::test_rasteriser_fill_rules, in both slots at different depths, and its back face
    c = Case("1-quad", 16, 16)
    c.rect(1, 4, 4, 12, 12, 0.5)
    c.rect(0, 2, 6, 6, 14, 0.75)
    c.tri(1, (0, 0, 0.5), (1024, 1024, 0.5), (1024, 0, 0.5), front=False)
    c.expect = [(4, 4, 0x01000001, 0x800000), (11, 11, 0x01000001, 0x800000), (12, 12, 0, 0xFFFFFF), (4, 11, 0x01000002, 0x800000), (3, 8, 1, 0xBFFFFF), (5, 8, 0x01000002, 0x800000)]
    out.append(c.filler())
    # fans of 3 to 8 triangles around a vertex that sits on a pixel centre: spokes in the eight directions run through pixel centres, so every
    # edge orientation has centres exactly on it; the hub and every spoke pixel is owned exactly once.  Sloped depth: the fan overlaps nothing.
    for W, H in ((16, 16), (64, 32)):
        c = Case("1-fans-%dx%d" % (W, H), W, H)
        hubs = [(3 + 8 * (n % 2) + (16 * ((n - 3) // 2) if W > 16 else 0), 3 + 8 * ((n // 2) % 2), n) for n in range(3, 9)]
        if W == 16:
            hubs = [(4, 4, 8), (11, 4, 3), (4, 11, 5), (11, 11, 6)]
        c.once_at = [(hx, hy) for hx, hy, _ in hubs]
        for k, (hx, hy, n) in enumerate(hubs):
            hub = (hx * 256 + 128, hy * 256 + 128, 0.3)
            use = DIRS8[:n] if n == 8 else [DIRS8[(j * 8) // n] for j in range(n)]
            rim = [(hub[0] + 3 * 256 * dx, hub[1] + 3 * 256 * dy, 0.7) for dx, dy in use]
            for j in range(n):
                a, b = rim[j], rim[(j + 1) % n]
                if (a[0] - hub[0]) * (b[1] - hub[1]) - (a[1] - hub[1]) * (b[0] - hub[0]) > 0:      # (a fan of 3 or 5 spokes has a reflex gap: left open)
                    c.tri(k & 1, hub, a, b)
        out.append(c.filler())
    # the eight edge orientations on their own: one thin triangle per direction whose long edges run through pixel centres
    c = Case("1-edges", 64, 32)
    for k, (dx, dy) in enumerate(DIRS8):
        x0, y0 = (8 + 16 * (k % 4)) * 256 + 128, (8 + 16 * (k // 4)) * 256 + 128
        a, b = (x0, y0, 0.3), (x0 + 5 * 256 * dx, y0 + 5 * 256 * dy, 0.6)      # (not 0.7: 0.3f + 0.7f = 1 exactly, z = 1/2 at the midpoint is a code on a tie)
        c.tri(k & 1, a, b, (x0 - 2 * 256 * dy, y0 + 2 * 256 * dx, 0.6))
        c.tri(k & 1, a, b, (x0 + 2 * 256 * dy, y0 - 2 * 256 * dx, 0.3))
    out.append(c.filler())
    # windings, zero area, no centre, slivers
    c = Case("1-degenerate", 64, 32)
    c.tri(0, (256, 256, 0.25), (2048, 256, 0.25), (256, 2048, 0.25), front=False)                       # back face
    c.tri(0, (256, 256, 0.5), (1280, 1280, 0.5), (2304, 2304, 0.5))                                     # three collinear vertices
    c.tri(0, (256, 256, 0.5), (256, 256, 0.5), (2304, 2304, 0.5))                                       # two equal vertices
    c.tri(1, (2048 + 140, 140, 0.5), (2048 + 250, 140, 0.5), (2048 + 140, 250, 0.5))                    # between four centres
    c.tri(1, (20 * 256 + 129, 256, 0.5), (20 * 256 + 383, 256, 0.5), (20 * 256 + 256, 290, 0.5))        # a box without a centre row
    c.tri(0, (512, 16 * 256 + 128, 0.3), (32 * 256 + 512, 20 * 256 + 128, 0.7), (32 * 256 + 512, 20 * 256 + 129, 0.7))   # slivers one sub-pixel wide across 30 pixels
    c.tri(1, (512, 4 * 256 + 128, 0.3), (512, 4 * 256 + 129, 0.3), (32 * 256 + 512, 4 * 256 + 128, 0.7))                 # ... with centres exactly on its upper edge
    c.tri(1, (40 * 256 + 128, 256, 0.7), (40 * 256 + 129, 256, 0.7), (40 * 256 + 128, 31 * 256, 0.3))                   # ... and vertical, centres on its left edge
    c.tri(0, (50 * 256 + 127, 256, 0.7), (50 * 256 + 128, 256, 0.7), (50 * 256 + 128, 31 * 256, 0.3))                   # ... centres on its right edge: none drawn
    c.tri(0, (48 * 256 + 64, 64, 0.5), (52 * 256 + 64.5, 64.5, 0.5), (48 * 256 + 64.5, 8 * 256 + 64.5, 0.5))            # half units: snapping ties (64 x 32: exact)
    out.append(c.filler())
    return out


# ---- family 2: watertight meshes ----------------------------------------------------------------------------------------------------------------
def _grid(c, cell, merged, seed, offset):
    """A jittered, triangulated grid that overhangs the frame; `merged` = (i0, j0, i1, j1) replaces a block of cells by two triangles whose border
    vertices are unjittered and therefore exactly on the big triangles' edges."""
    rng = np.random.RandomState(seed)
    nx, ny = c.W // cell + 3, c.H // cell + 3
    P = {}
    for j in range(ny + 1):
        for i in range(nx + 1):
            X, Y = (i - 1) * cell * 256, (j - 1) * cell * 256
            on_border = merged and merged[0] <= i <= merged[2] and merged[1] <= j <= merged[3]
            if not on_border:
                X += int(rng.randint(-cell * 60, cell * 60)) + offset
                Y += int(rng.randint(-cell * 60, cell * 60)) + offset
            P[i, j] = (X, Y, (0.3, 0.7, 0.45, 0.6)[(i + 2 * j) % 4])
    for j in range(ny):
        for i in range(nx):
            if merged and merged[0] <= i < merged[2] and merged[1] <= j < merged[3]:
                continue
            a, b, cc, d = P[i, j], P[i + 1, j], P[i + 1, j + 1], P[i, j + 1]
            inst = (i + j) & 1
            if (i ^ j) & 1:
                c.tri(inst, a, b, cc); c.tri(inst, a, cc, d)
            else:
                c.tri(inst, a, b, d); c.tri(inst, b, cc, d)
    if merged:
        a, b, cc, d = P[merged[0], merged[1]], P[merged[2], merged[1]], P[merged[2], merged[3]], P[merged[0], merged[3]]
        c.tri(0, a, b, cc); c.tri(1, a, cc, d)
    c.once = True
    return c.filler()


def watertight_cases():
    return [_grid(Case("2-grid-64x32", 64, 32), 8, None, 1, 0.5),
            _grid(Case("2-grid-97x61", 97, 61), 8, None, 2, 0.25),
            _grid(Case("2-grid-large-64x32", 64, 32), 8, (2, 1, 8, 5), 3, 0.5),
            _grid(Case("2-grid-large-97x61", 97, 61), 8, (3, 2, 10, 8), 4, 0.25)]


# ---- family 3: the small/large threshold --------------------------------------------------------------------------------------------------------
def threshold_cases():
    out = []
    # constant z per triangle, distinct per pair, nearer in front: overlaps are decided by depth, ties by word
    c = Case("3-boxes-48x48", 48, 48)
    c.rect(0, 0, 0, 32, 32, 0.5)          # 1024: small
    c.rect(1, 8, 8, 41, 39, 0.5625)       # 33 x 31 = 1023: small
    c.rect(0, 4, 20, 45, 45, 0.625)       # 41 x 25 = 1025: large
    c.rect(1, 16, 0, 48, 32, 0.5)         # 1024 again, equal depth with the first pair: instance 0 keeps the overlap
    c.rect(1, -10, -10, 32, 32, 0.75)     # 42 x 42 cut to 32 x 32 = 1024 by the frame
    c.rect(0, 20, 20, 60, 60, 0.875)      # cut to 28 x 28
    c.rect(0, 0, 0, 5, 48, 0.25); c.rect(1, 6, 0, 13, 48, 0.25); c.rect(0, 14, 1, 45, 34, 0.28125)     # widths 5, 7, 31 (31 x 33 = 1023)
    out.append(c.filler())
    # boxes cut to 1024 pixels or fewer only by the strip clamp: strips (40, 45) and (40, 47) of 96 rows give the kernels rows 22 .. 63 and
    # 22 .. 65, 41 and 43 rows, so the 24 columns of the first pair are 984 candidates (small) in one strip and 1032 (large) in the other
    c = Case("3-boxes-48x96-strip", 48, 96, strips=[(40, 45), (40, 47)])
    c.rect(0, 0, 0, 24, 96, 0.5)
    c.rect(1, 20, 0, 45, 96, 0.25)        # 25 columns: 1025 and 1075, large in both
    c.rect(0, 30, 30, 48, 70, 0.125)      # 18 x 40 = 720 in the frame, 18 x 33 = 594 and 18 x 35 = 630 in the strips
    c.strip_lanes = {(40, 45): {0: 984, 1: 984, 2: 594, 3: 594, 4: 0, 5: 0}, (40, 47): {0: 0, 1: 0, 2: 630, 3: 630, 4: 0, 5: 0}}
    out.append(c.filler())
    c = Case("3-boxes-1056x4", 1056, 4)
    c.rect(0, 0, 0, 1024, 1, 0.5)         # 1024 x 1
    c.rect(1, 16, 1, 1039, 2, 0.5)        # 1023 x 1
    c.rect(0, 31, 1, 1056, 2, 0.75)       # 1025 x 1: large
    c.rect(1, 3, 2, 515, 4, 0.5)          # 512 x 2
    c.rect(0, 700, 1, 1041, 4, 0.25)      # 341 x 3 = 1023
    c.rect(1, 10, 3, 693, 4, 0.375)       # 683 x 1
    c.rect(0, 0, -5, 300, 3, 0.625)       # 300 x 8 cut to 300 x 3 by the frame
    out.append(c.filler())
    c = Case("3-boxes-4x1056", 4, 1056)
    c.rect(0, 0, 0, 1, 1024, 0.5)         # 1 x 1024: every row of the box beyond the 256th
    c.rect(1, 1, 16, 2, 1039, 0.5)        # 1 x 1023
    c.rect(0, 1, 31, 2, 1056, 0.75)       # 1 x 1025: large
    c.rect(1, 2, 3, 4, 515, 0.5)          # 2 x 512
    c.rect(0, 1, 700, 4, 1041, 0.25)      # 3 x 341
    c.rect(1, 0, 100, 4, 356, 0.875)      # 4 x 256
    out.append(c.filler())
    return out


# ---- family 4: wave work sharing ----------------------------------------------------------------------------------------------------------------
def _zero(c, inst, kind, k):
    """A triangle that leaves its lane without candidates, in every way rasterSmall has."""
    x, y, z = (k * 7) % 60, (k * 5) % 28, 0.125
    if kind == 0:
        return c.tri(inst, (x * 256, y * 256, z), ((x + 3) * 256, y * 256, z), (x * 256, (y + 3) * 256, z), front=False)      # back face
    if kind == 1:
        return c.tri(inst, (x * 256, y * 256, z), ((x + 1) * 256, (y + 1) * 256, z), ((x + 3) * 256, (y + 3) * 256, z))       # zero area
    if kind == 2:
        return c.tri(inst, ((c.W + 2) * 256, y * 256, z), ((c.W + 9) * 256, y * 256, z), ((c.W + 2) * 256, (y + 3) * 256, z)) # off screen
    if kind == 3:
        return c.tri(inst, (x * 256, -9 * 256, z), ((x + 3) * 256, -9 * 256, z), (x * 256, -2 * 256, z))                      # above the frame
    if kind == 4:
        return c.raw(inst, (np.nan, 0.0, z), (0.5, 0.0, z), (0.0, -0.5, z))                                                    # NaN
    if kind == 5:
        return c.raw(inst, (0.0, 0.0, z), (np.inf, 0.0, z), (0.0, -0.5, z))                                                    # inf
    if kind == 6:
        return c.raw(inst, (0.0, 0.0, z), (0.5, -np.inf, z), (0.0, -0.5, np.nan))
    if kind == 7:
        return c.tri(inst, (x * 256 + 140, y * 256 + 140, z), (x * 256 + 250, y * 256 + 140, z), (x * 256 + 140, y * 256 + 250, z))    # a box without a centre
    if kind == 8:
        # w = 0 on a vertex in front of the near plane and inside the guard band (clip = (0, 0, 1/4, 0)): not clipped, not snapped, dropped
        return c.raw(inst, (0.0, 0.0, 0.0), (0.5, 0.0, 1.0), (0.0, -0.5, 1.0))
    return c.corner(inst, x, (1 + k % 2) if k & 2 else (59 + k % 2), 3, 3, z)                                                      # inside the frame, outside the rows the pass gets for STRIP


SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16, 18, 20, 21, 24, 25, 27, 28, 30, 32, 35, 36, 40]


STRIP = (24, 40)          # of 64 rows: the kernels get rows 6 .. 58


def wave_case(nt0, name, persp=False, strip=False):
    """One list of 1164 triangles (18 full waves and a wave of 12: five workgroups, the last wave partly past the end), split into the two
    instances at nt0.  Depth is constant per triangle and taken from 64 values (three under the perspective transform), so the frame is full
    of ties that the lower word wins.  persp: both instances go through clip = (x, y, z / 4 + 1 / 4, z), which adds the zero "w <= 0";
    strip: 64 rows, of which the pass draws 6 .. 58 (the strip and its apron), which adds the zero "outside the pass's rows" and cuts the boxes
    that reach beyond them."""
    H = 64 if strip else 32
    c = Case(name, 64, H, strips=[STRIP] if strip else None, wvp=(perspective(0.25, 0.25),) * 2 if persp else (IDENTITY, IDENTITY))
    if persp:
        c.levels = (1.0, 2.0, 4.0)
    kinds = list(range(8)) + ([8] if persp else []) + ([9] if strip else [])
    plan = []                                                  # candidate count per triangle, 0: one of the zeros
    plan += [0] + [1 + (k % 5) for k in range(63)]             # wave 0: zero at lane 0
    plan += [1 + (k % 7) for k in range(63)] + [0]             # wave 1: zero at lane 63
    plan += [0 if k & 1 else 6 for k in range(64)]             # wave 2: alternating
    plan += [0] * 63 + [1024]                                  # wave 3: 63 zeros, then one box of 1024
    plan += [0] * 64                                           # wave 4: no candidates at all
    plan += [1] * 64                                           # wave 5: 64 in total
    plan += [2] * 64                                           # wave 6: 128
    plan += [1024] * 64                                        # wave 7: 65536
    for w in range(8, 18):                                     # mixed: runs of zeros of every kind among boxes of every small size
        plan += [0 if (k * (w - 5)) % 11 < 4 else SIZES[(k * w) % len(SIZES)] for k in range(64)]
    plan += [3, 0, 0, 12, 1, 0, 30, 1025, 0, 2, 0, 9]          # wave 18: 12 triangles, the rest of the wave past the end; one goes to the tile pass
    assert len(plan) == 1164
    zeros = 0
    c.lanes, in_strip = {}, {}
    kr = kernel_rows(STRIP, H)
    rows = lambda y, h: max(0, min(y + h, kr[1]) - max(y, kr[0]))
    for t, n in enumerate(plan):
        inst = 0 if t < nt0 else 1
        z = (1 + (t * 37) % 64) / 128.0
        if n == 0:
            kind = kinds[zeros % len(kinds)]; zeros += 1
            _zero(c, inst, kind, t)
            c.lanes[t], in_strip[t] = (9 if kind == 9 else 0), 0
            continue
        if n == 1:
            x, y, w, h = (t * 13) % 64, (t * 7) % H, 1, 1
            c.dot(inst, x, y, z)
        else:
            w = (32 if n == 1024 else 41) if n >= 1024 else next(w for w in (8, 7, 6, 5, 4, 3, 2, 1) if n % w == 0)
            h = n // w
            x, y = ((t * 5) % (64 - w), (t % 33) if strip else 0) if n >= 1024 else ((t * 11) % (64 - w), (t * 3) % (H - h))
            c.corner(inst, x, y, w, h, z)
        c.lanes[t] = n if n <= SMALL_BOX else 0
        in_strip[t] = w * rows(y, h)
    if strip:
        c.strip_lanes = {STRIP: in_strip}
    else:
        c.wave_totals = {4: 0, 5: 64, 6: 128, 7: 65536, 3: 1024}
    return c


def wave_cases():
    # the two instances meet at lanes 1, 32 and 63 of a wave, at a wave boundary and at a workgroup boundary
    return [wave_case(64 * 9 + 1, "4-waves-lane1"), wave_case(64 * 2 + 32, "4-waves-lane32"), wave_case(64 * 7 + 63, "4-waves-lane63"),
            wave_case(64 * 7, "4-waves-wave-boundary"), wave_case(256 * 2, "4-waves-workgroup-boundary"),
            wave_case(64 * 9 + 1, "4-waves-perspective", persp=True), wave_case(64 * 2 + 32, "4-waves-strip", strip=True)]


# ---- family 5: depth resolve --------------------------------------------------------------------------------------------------------------------
def depth_cases():
    out = []
    for order in ("equal", "increasing", "decreasing"):
        c = Case("5-coincident-%s" % order, 16, 16)
        for t in range(512):
            z = {"equal": 0.5, "increasing": (t + 1) / 1024.0, "decreasing": (512 - t) / 1024.0}[order]
            c.corner(t // 256, 2, 2, 12, 12, z)
        first = 1 if order != "decreasing" else 0x01000000 + 256
        c.expect = [(2, 2, first, None), (7, 5, first, None), (13, 13, 0, 0xFFFFFF)]
        out.append(c)
    c = Case("5-codes", 16, 16)
    c.rect(1, 0, 0, 8, 8, 0.5); c.rect(0, 4, 4, 12, 12, 0.5)                                  # equal depth across instances: instance 0 wins
    c.rect(0, 12, 0, 14, 2, 0.0)                                                              # code 0
    c.rect(0, 14, 0, 16, 2, 2.0 ** -24)                                                       # code 1
    c.rect(1, 12, 2, 14, 4, 1.0 - 2.0 ** -24)                                                 # code 0xFFFFFE
    c.rect(1, 14, 2, 16, 4, 1.0)                                                              # z = 1: code 0xFFFFFF does not beat the cleared key
    c.rect(0, 12, 4, 16, 6, 1.0); c.rect(1, 12, 4, 14, 6, 1.0 - 2.0 ** -24)                   # ... and is not there to be beaten either
    # z = 9/16 at the centre of pixel 0, 25/16 at the centre of pixel 16: cut per pixel at z <= 1, the centre of pixel 7 has z = 1 exactly
    # (not from 1/2: z = 1/2 is a code on a tie, and this triangle is sloped)
    c.tri(1, (128, 12 * 256, 0.5625), (128 + 4096, 12 * 256, 1.5625), (128, 16 * 256, 0.5625)); c.tri(1, (128 + 4096, 12 * 256, 1.5625), (128 + 4096, 16 * 256, 1.5625), (128, 16 * 256, 0.5625))
    c.expect = [(5, 5, 1, 0x800000), (2, 2, 0x01000001, 0x800000), (12, 0, None, 0), (15, 1, None, 1), (13, 3, None, 0xFFFFFE), (15, 3, 0, 0xFFFFFF), (15, 5, 0, 0xFFFFFF),
                (13, 5, None, 0xFFFFFE), (0, 13, 0x01000001 + 8, 0x8FFFFF), (6, 13, 0x01000001 + 8, None), (6, 15, 0x01000001 + 9, None), (7, 13, 0, 0xFFFFFF), (8, 13, 0, 0xFFFFFF)]
    out.append(c)
    # equal depth between a small and a large triangle, in both index orders and across the instances (48 x 48: the smallest frame with a large box)
    c = Case("5-small-large", 48, 48)
    c.rect(0, 0, 0, 8, 8, 0.5); c.rect(0, 0, 0, 40, 40, 0.5); c.rect(0, 30, 30, 38, 38, 0.5)
    c.rect(1, 4, 4, 44, 44, 0.5); c.rect(1, 40, 2, 46, 8, 0.5); c.rect(1, 0, 0, 48, 48, 0.5)
    c.expect = [(2, 2, 1, 0x800000), (20, 10, 3, 0x800000), (34, 34, 3, 0x800000), (42, 42, 0x01000001, None), (44, 4, 0x01000001 + 2, None), (47, 47, 0x01000001 + 4, None)]
    out.append(c)
    return out


# ---- family 6: clipping -------------------------------------------------------------------------------------------------------------------------
def clip_cases():
    """32 x 16.  Both instances go through clip = (x, y, z - 1/2, z): a vertex at z = 1 has w = 1 and depth 1/2, one at z = 0 lies behind the near
    plane at z_clip = -1/2, w = 0, so an edge between them is cut at t = 1/2.  Guard-band cuts run from x = 0 to x = 512 w (t = 1/2 again)."""
    out = []
    P = perspective(1.0, -0.5)
    c = Case("6-near", 32, 16, wvp=(P, P))
    a = c.raw(0, (-0.5, 0.5, 1.0), (0.5, 0.5, 1.0), (-0.5, -1.5, 0.0))            # one vertex behind: a quad, fan of two
    b = c.raw(1, (0.5, -0.25, 1.0), (1.75, 0.75, 0.0), (0.75, -1.75, 0.0))        # two behind: a triangle
    d = c.raw(1, (-1.0, 1.0, 0.0), (1.0, 1.0, 0.0), (0.0, -1.0, 0.0))             # all three behind: nothing
    e = c.raw(0, (-0.75, 0.875, 1.0), (0.25, 0.875, 1.0), (0.0, -0.125, 0.0))     # one behind, a band one pixel high
    c.polygons = {(0, a): 4, (1, b): 3, (1, d): 0, (0, e): 4}
    c.clipped = 4
    out.append(c.filler())
    # one vertex behind, placed so that the quad is the square of pixel corners (4, 2) .. (12, 10) and the fan's inner diagonal runs through
    # the centres of pixels (4, 2) .. (11, 9): each is owned by exactly one of the two fan triangles.  The second quad, 16 pixels to the
    # right, starts at another vertex, so its fan is cut along the other diagonal, (27, 2) .. (20, 9).  (Corners, not centres: z is 1/2 on the
    # quad's upper edge, a code on a tie, and no centre may lie there.)
    c = Case("6-near-diagonal", 32, 16, wvp=(P, P))
    a = c.raw(0, (-0.75, 0.75, 1.0), (-0.25, 0.75, 1.0), (0.0, -1.0, 0.0))
    b = c.raw(1, (0.75, 0.75, 1.0), (0.0, -1.0, 0.0), (0.25, 0.75, 1.0))
    c.polygons = {(0, a): 4, (1, b): 4}
    c.clipped = 2
    c.once_at = [(4 + j, 2 + j) for j in range(8)] + [(27 - j, 2 + j) for j in range(8)] + [(4, 9), (11, 2), (20, 2), (27, 9)]
    c.expect = [(8, 6, 1, None), (24, 6, 0x01000001, None), (3, 6, 0, None), (12, 6, 0, None), (19, 6, 0, None), (28, 6, 0, None)]
    c.drawn = 128
    out.append(c.filler())
    c = Case("6-guard", 32, 16)
    g1 = c.raw(0, (0.0, 0.5, 0.25), (512.0, 0.0, 0.25), (0.0, -0.5, 0.25))          # one plane
    g2 = c.raw(1, (0.0, 0.0, 0.5), (0.0, 512.0, 0.5), (512.0, 0.0, 0.5))            # two adjacent planes
    g3 = c.raw(1, (-0.5, -0.5, 0.75), (-0.5, 256.0, 0.75), (256.0, -0.5, 0.75))     # vertices exactly at x = 256 w, y = 256 w: inside, not clipped
    g4 = c.raw(0, (300.0, 0.5, 0.125), (600.0, 0.5, 0.125), (300.0, -0.5, 0.125))   # beyond the plane altogether
    g5 = c.raw(0, (200.0, 0.5, 0.125), (600.0, 0.5, 0.125), (200.0, -0.5, 0.125))   # straddles the plane, not the viewport
    g6 = c.raw(1, (-384.0, -128.0, 0.875), (-128.0, 512.0, 0.875), (512.0, -384.0, 0.875))   # all four planes: seven vertices
    g7 = c.raw(0, (-0.75, -0.5, 0.875), (-0.5, -0.5, 0.875), (-0.75, -1.0, 0.875))        # an unclipped small triangle that ties with g6 (tile pass) and has the lower word
    g8 = c.raw(1, (-0.75, 0.5, 0.875), (-0.5, 0.5, 0.875), (-0.75, 0.0, 0.875))     # ... and one with the higher word
    c.polygons = {(0, g1): 4, (1, g2): 5, (0, g4): 0, (0, g5): 4, (1, g6): 7}
    c.clipped = 5
    c.expect = [(4, 12, 4, 0xDFFFFF), (5, 5, 0x01000003, 0xDFFFFF), (20, 8, 1, 0x400000)]
    out.append(c.filler())
    return out


# ---- family 7: frames and strips ----------------------------------------------------------------------------------------------------------------
def _scatter(c, seed, n):
    """Constant-z triangles of every size all over the frame, depths from 48 values (ties included), a quarter of a sub-pixel unit off the grid
    where the frame size is no power of two."""
    rng = np.random.RandomState(seed)
    off = 0.5 if (c.W & (c.W - 1)) == 0 and (c.H & (c.H - 1)) == 0 else 0.25
    for k in range(n):
        span = (4, 20, 80, 2 * max(c.W, c.H))[k % 4] * 256
        cx, cy = int(rng.randint(0, c.W * 256)), int(rng.randint(0, c.H * 256))
        p = [(cx + int(rng.randint(-span, span + 1)) + (off if k % 3 == 0 else 0), cy + int(rng.randint(-span, span + 1)) + (off if k % 5 == 0 else 0)) for _ in range(3)]
        z = (1 + int(rng.randint(0, 48))) / 64.0
        c.tri(k & 1, *[(x, y, z) for x, y in p])
    return c


def frame_cases():
    out = []
    c = Case("7-1x1", 1, 1)
    c.tri(0, (0, 0, 0.5), (512, 0, 0.5), (0, 512, 0.5)); c.tri(1, (0, 0, 0.25), (256, 256, 0.25), (0, 256, 0.25)); c.tri(1, (-2560, -2560, 0.125), (-256, -2560, 0.125), (-2560, 40, 0.125))
    c.expect = [(0, 0, 1, 0x800000)]
    out.append(c)
    for W, H in ((65, 17), (333, 7)):
        out.append(_scatter(Case("7-scatter-%dx%d" % (W, H), W, H), W, 60).filler())
        c = Case("7-sloped-%dx%d" % (W, H), W, H)
        # sloped depth over the whole frame, as two triangles that share the diagonal and lie alone
        c.tri(0, (0.25, 0.25, 0.3), (W * 256 + 77, -33, 0.7), (-51, H * 256 + 20, 0.45)); c.tri(1, (W * 256 + 77, -33, 0.7), (W * 256 + 5.25, H * 256 + 9, 0.6), (-51, H * 256 + 20, 0.45))
        c.once = True
        out.append(c)
    # 8192 columns, the width the contract's guard-band bound is stated for: triangles at the far right, one across the full width (large), boxes of 1024 x 1 and 512 x 2 at the right end
    c = Case("7-8192x2", 8192, 2)
    c.tri(0, (0, 0, 0.75), (8192 * 256, 0, 0.75), (0, 512, 0.75)); c.tri(1, (8192 * 256, 0, 0.75), (8192 * 256, 512, 0.75), (0, 512, 0.75))
    c.rect(0, 8192 - 1024, 0, 8192, 1, 0.5); c.rect(1, 8192 - 512, 0, 8192, 2, 0.625); c.dot(1, 8191, 1, 0.25); c.dot(0, 8191, 0, 0.25); c.dot(0, 8128, 1, 0.25); c.dot(1, 8127, 0, 0.25)
    c.rect(1, 8000, 0, 8200, 1, 0.375); c.dot(0, 0, 0, 0.25); c.dot(1, 4095, 1, 0.25); c.dot(1, 4096, 0, 0.25)
    out.append(c)
    # strips on 97 x 61, with triangles across rasterLarge's block borders (x = 63 | 64, rows 15 | 16 counted from the pass's first row, which is the strip's minus 18) and single
    # pixels on each of the four rows a lane owns; the rows of the strip are compared
    strips = [(0, 61), (5, 23), (16, 17), (60, 61), (37, 50)]      # the pass's first rows: 0, 0, 0, 42, 19
    c = _scatter(Case("7-strips-97x61", 97, 61, strips=strips), 97, 80)
    for r0 in sorted({kernel_rows(strip, 61)[0] for strip in strips}):
        for dy in (14, 15, 16, 17):
            c.dot((r0 + dy) & 1, 63 if dy & 1 else 64, min(r0 + dy, 60), 0.0078125)
        for k in range(4):
            c.dot(k & 1, 60 + k, min(r0 + k, 60), 0.0078125); c.dot(k & 1, 66 + k, min(r0 + 4 + k, 60), 0.0078125)
        c.rect(0, 60, min(r0 + 13, 57), 68, min(r0 + 13, 57) + 4, 0.01171875)          # small, across both borders
        c.rect(1, 30, r0 - 2, 96, min(r0 + 18, 61), 0.015625)                          # large, across both borders
    out.append(c)
    return out


# ---- family 8: the full large-triangle queue ----------------------------------------------------------------------------------------------------
def overflow_case():
    """65536 + 256 + 8 triangles whose boxes all exceed 1024 pixels on 64 x 32: more than the queue holds, so 264 of them -- which ones depends
    on scheduling -- are rasterised in place by rasterSmall.  Constant z each.  The first 256 are nested right triangles in the upper right half
    (the vertex on the top edge moves right by 28 sub-pixel units per triangle, depth falling with it: each wins the sliver its predecessor does
    not cover), the last 256 the same in the lower left half, the 65288 between them repeat four big triangles at depths behind both and win
    the two-pixel gap the others leave."""
    c = Case("8-overflow", 64, 32)
    W, H = 64 * 256, 32 * 256
    total = LARGE_CAPACITY + 256 + 8
    for t in range(total):
        inst = 0 if t < total // 2 else 1
        if t < 256:
            z = 0.5 - t / 1024.0
            c.tri(inst, (512 + 28 * t, 0, z), (W, 0, z), (W, H, z))
        elif t >= total - 256:
            k = t - (total - 256)
            z = 0.5 - k / 1024.0
            c.tri(inst, (0, 0, z), (W - 512 - 28 * k, H, z), (0, H, z))
        else:
            z = 0.75 + (t % 4) / 64.0
            k = t % 4
            if k == 0: c.tri(inst, (0, 0, z), (W, 0, z), (W, H, z))
            elif k == 1: c.tri(inst, (0, 0, z), (W, H, z), (0, H, z))
            elif k == 2: c.tri(inst, (0, 0, z), (W, 0, z), (0, H, z))
            else: c.tri(inst, (W, 0, z), (W, H, z), (0, H, z))
    c.winners = [(0, 256, 64), (total - 256, total, 64), (256, total - 256, 1)]
    c.large_at_least = total
    return c


# ---- family 9: tile words -----------------------------------------------------------------------------------------------------------------------
def tile_case(kind, last=((24, 60), (3, 59), (72, 35), (21, 54), (74, 46))):
    """97 x 61: scenes that touch a 16 x 16 tile in exactly one pixel -- each corner of a tile, the last partial tile column and row -- through a
    small triangle, a large one (a sliver whose box exceeds 1024 pixels but which covers one centre) or the overflow path (the same sliver behind
    65536 queued ones).  Tiles are counted from the pass's first row, the strip's minus 18: 0 for strips (0, 61) and (5, 50), 17 for (35, 61),
    where at least two of the last five spots (`last`, found by search for the sliver kinds, whose other slivers smear over many tiles) lie in
    tiles that an index without that row would leave unmarked: check() asserts it."""
    c = Case("9-tiles-%s" % kind, 97, 61, strips=[(0, 61), (5, 50), (35, 61)])
    c.tile_strips = [(35, 61)]
    spots = [(16, 16), (31, 16), (16, 31), (31, 31), (96, 3), (96, 60), (40, 60), (64, 21), (79, 36), (3, 5), (50, 49), (81, 20), (95, 52),
             ] + list(last)
    for k, (x, y) in enumerate(spots):
        inst = 1 if kind == "overflow" else k & 1
        if kind == "small":
            c.dot(inst, x, y, 0.5)
        else:
            # a sliver whose blunt end just holds the pixel's centre and which leaves the centre's row at once: its box holds more than 1024 pixels
            cx, cy = x * 256 + 128, y * 256 + 128
            sx, sy = (-1 if x >= 48 else 1), (-1 if y >= 30 else 1)
            # (the spots of the last strip: z climbs to 300 along the sliver, so the depth clip leaves nothing of it but the spot -- it draws
            # into no other tile, and lies alone as a sloped triangle must)
            c.tri(inst, (cx - 20 * sx, cy - 3, 0.5), (cx - 20 * sx, cy + 3, 0.5), (cx + sx * 400 * 256, cy + sy * 40 * 256, 300.0 if k >= 13 else 0.5))
    if kind != "small":
        c.large_at_least = len(spots)
    if kind == "overflow":
        # the queue is full before the slivers (the last triangles of instance 1, in the last workgroup) are likely to arrive: 65536 slivers
        # behind them, each with a box of 41 x 55 pixels (41 x 43 in the rows of the last strip), 128 copies of each of 512 places
        for k in range(512):
            x0, y0 = (2 + k % 32) * 256, 512 + 64 * (k // 32)
            c.tri(0, (x0, y0, 0.75), (x0 + 40 * 256, y0 + 55 * 256, 0.75), (x0 + 39 * 256, y0 + 55 * 256, 0.75))
        c.i[0] = c.i[0] * (LARGE_CAPACITY // 512)
        c.large_at_least += LARGE_CAPACITY
    return c.filler()


HEAVY = {"9-tiles-overflow": lambda: tile_case("overflow"), "8-overflow": overflow_case}      # more than 65536 triangles each: built when first asked for
_CACHE = {}


def names():
    if "light" not in _CACHE:
        light = fill_rule_cases() + watertight_cases() + threshold_cases() + wave_cases() + depth_cases() + clip_cases() + frame_cases()
        light += [tile_case("small"), tile_case("large")]
        _CACHE["light"] = [c.name for c in light]
        _CACHE.update((c.name, c) for c in light)
        assert len(_CACHE) == len(light) + 1
    return _CACHE["light"] + list(HEAVY)


def case(name):
    """The case of that name, built once per process and left unchanged."""
    names()
    if name not in _CACHE:
        _CACHE[name] = HEAVY[name]()
    return _CACHE[name]
