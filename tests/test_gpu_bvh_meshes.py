"""The device BVH (csrc/lbvh.hip: Morton codes, radix sort, PLOC, refit schedule, 4-wide collapse, LDS top table) and the
trace kernel that walks it (csrc/trace.hip: LDS stack with global spill, work sharing, tie rule) on synthetic meshes chosen for
where builders and traversals go wrong: sizes on either side of the build's thresholds (PLOC radius 16, 256-thread blocks,
RT_PLOC_STOP 2048, RT_PLOC_LDS 3072, RT_TREELET_NODES 1024, top tables of 16 and 96 nodes), equal boxes and Morton codes, a zero
extent, zero-area and sliver triangles, a tree whose traversal stack spills, rays through shared edges and vertices, axis-aligned
and in-plane rays, hits exactly at tmin / tmax, ties between instances.

Every case is checked three ways: the trees' structure (tests/bvh_checks.py, leaf vertices included), the closest hits of the HIP
traversal against the oracle's BRUTE-FORCE loop over all triangles (no tree at all: a hit a bad tree loses shows), and against the
oracle walking the device's own arrays.  Instance, primitive, t and barycentrics bit for bit."""
import math

import numpy as np
import pytest

from bvh_cases import grid_mesh, mesh_from_tris, rays_through_box, soup, world
from gpu_support import Scene, interval_edges, model_box

pytestmark = pytest.mark.gpu

RT_STACK = 16            # LDS entries of the trace kernel's per-lane stack (csrc/trace.hip); deeper entries spill to global memory
EMPTY = 0x7FFFFFFF       # RT_BVH4_EMPTY


SMALL0 = mesh_from_tris(soup(12, seed=100))      # the ground slot's mesh where a case is about the model's


# ---- triangle soups across the build's thresholds ------------------------------------------------------------------------------
SIZES = [1, 2, 3, 5, 16, 17, 32, 33, 34, 96, 97, 255, 256, 257, 1024, 1025, 1026, 2048, 2049, 3072, 3073, 40000]


@pytest.mark.parametrize("n", SIZES)
def test_random_soup_in_the_model_slot(built, n):
    s = Scene(SMALL0, mesh_from_tris(soup(n, seed=n)), world1=world(1.0, (0.25, 0.5, -0.125), rot_y90=(n % 2 == 1)))
    try:
        lo, hi = model_box(s)
        rays = rays_through_box(lo, hi, 3000 if n < 10000 else 1500, seed=n)
        s.compare(rays, "soup of %d" % n, min_hits=1)
        interval_edges(s, rays[:500], "soup of %d" % n)
    finally:
        s.close()


@pytest.mark.parametrize("n", [1, 2, 13, 17, 33, 97, 257, 1025, 3073])
def test_random_soup_in_the_ground_slot(built, n):
    """Slot 0 holds 12 triangles in the sample: its top table of 16 nodes has never been full.  Here it is, beside a model that
    overlaps it (rays meet both instances; equal t would go to instance 0)."""
    s = Scene(mesh_from_tris(soup(n, seed=1000 + n)), mesh_from_tris(soup(300, seed=7)),
              world0=world(2.0, (0.5, 0.0, 0.0)), world1=world(1.0, (0.0, 0.0, 0.5)))
    try:
        if n >= 97:
            assert s.tops[0] == 16, "the ground's table holds %d nodes" % s.tops[0]
        lo, hi = model_box(s, 0)
        s.compare(rays_through_box(lo, hi, 3000, seed=n), "ground soup of %d" % n, min_hits=1)
    finally:
        s.close()


# ---- degenerate meshes ----------------------------------------------------------------------------------------------------------
def test_coincident_triangles(built):
    """3000 copies of one triangle: equal boxes, equal Morton codes.  With a tie rule that is not an order on pairs PLOC merges one
    pair per round (a caterpillar 3000 levels deep: the build fails "deeper than 128 levels" / "more than 1024 rounds"); with
    lbvh.hip plocPairKey the run pairs up level by level.  Every ray that hits, hits all 3000 at the same t: primitive 0."""
    n = 3000
    tri = np.array([[-1.0, -0.5, 0.25], [1.0, -0.25, -0.25], [0.125, 1.0, 0.0]], np.float32)
    s = Scene(SMALL0, mesh_from_tris(np.repeat(tri[None], n, axis=0)))
    try:
        assert s.depth[1] <= 2 * math.ceil(math.log2(n)) + 4, "tree of %d coincident triangles is %d levels deep" % (n, s.depth[1])
        b = s.compare(rays_through_box(tri.min(axis=0), tri.max(axis=0), 3000, seed=3), "coincident", min_hits=500)
        assert (b["prim"][b["valid"] & (b["inst"] == 1)] == 0).all()
    finally:
        s.close()


def test_zero_area_triangles_at_one_point_among_normal_ones(built):
    rng = np.random.default_rng(4)
    p = np.array([0.125, 0.25, -0.375], np.float32)
    tris = np.concatenate([np.repeat(np.repeat(p[None, None], 3, axis=1), 2000, axis=0), soup(600, seed=5)])
    tris = tris[rng.permutation(len(tris))]
    s = Scene(SMALL0, mesh_from_tris(tris))
    try:
        lo, hi = model_box(s)
        rays = rays_through_box(lo, hi, 2500, seed=6)
        toward = rays[:500].copy(); toward[:, 3:6] = p - toward[:, :3]      # straight at the degenerate point
        s.compare(np.concatenate([rays, toward]), "zero-area", min_hits=1)
    finally:
        s.close()


def test_every_triangle_twice_with_reversed_winding(built):
    """Every hit meets primitives i and i + n, the same triangle wound both ways: t may differ in its last bit (the edge functions
    come in another order), then the lower id wins -- the same one on every side."""
    t = soup(1500, seed=8)
    s = Scene(SMALL0, mesh_from_tris(np.concatenate([t, t[:, [0, 2, 1]]])))
    try:
        lo, hi = model_box(s)
        s.compare(rays_through_box(lo, hi, 3000, seed=9), "reversed winding", min_hits=300)
    finally:
        s.close()


def test_flat_grid_shared_edges_vertices_and_axis_aligned_rays(built):
    q, step = 128, 0.125
    v, idx = grid_mesh(q, step)
    s = Scene(SMALL0, (v, idx), world0=world(1.0, (0.0, 100.0, 0.0)))      # (the ground's soup out of the way, above)
    try:
        rng = np.random.default_rng(10)
        half = q / 2 * step
        # random rays through the grid
        s.compare(rays_through_box((-half, -0.5, -half), (half, 0.5, half), 3000, seed=11), "grid: random", min_hits=500)
        # aimed exactly at grid vertices (up to six triangles meet) and at midpoints of shared edges (two meet), from random origins
        n = 1500
        vert = v[rng.integers(0, len(v), n), :3].astype(np.float64)
        a = rng.integers(0, q, (n, 2)); axis = rng.integers(0, 3, n)      # edge along x, along z, or the quad's diagonal
        mid = np.stack([(a[:, 0] - q / 2 + np.where(axis != 1, 0.5, 0.0)) * step, np.zeros(n),
                        (a[:, 1] - q / 2 + np.where(axis != 0, 0.5, 0.0)) * step], 1)
        for name, tgt in (("vertices", vert), ("edge midpoints", mid)):
            org = tgt + np.stack([rng.uniform(-3, 3, n), rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 4, n), rng.uniform(-3, 3, n)], 1)
            rays = np.concatenate([org, tgt - org, np.zeros((n, 1)), np.full((n, 1), 1e30)], 1).astype(np.float32)
            s.compare(rays, "grid: aimed at " + name, min_hits=n // 2)
            interval_edges(s, rays[:300], "grid: aimed at " + name)
        # axis-aligned: straight down / up through vertices, edges and quads, with -0.0 direction components; origins on box planes
        n = 1200
        xz = np.stack([rng.integers(-q // 2, q // 2 + 1, n) * step / rng.choice([1, 2, 4], n),
                       rng.integers(-q // 2, q // 2 + 1, n) * step / rng.choice([1, 2, 4], n)], 1).astype(np.float32)
        y0 = rng.choice([1.0, 0.125, -2.0], n).astype(np.float32)
        down = np.zeros((n, 8), np.float32)
        down[:, 0], down[:, 1], down[:, 2] = xz[:, 0], y0, xz[:, 1]
        down[:, 3] = np.where(rng.random(n) < 0.5, -0.0, 0.0); down[:, 5] = np.where(rng.random(n) < 0.5, -0.0, 0.0)
        down[:, 4] = np.where(y0 > 0, -1.0, 1.0)
        down[:, 7] = 1e30
        s.compare(down, "grid: axis-aligned", min_hits=n // 2)
        interval_edges(s, down[:300], "grid: axis-aligned")
        # axis-aligned along x and z, from origins on the grid's box planes and off them (these lie in or beside the plane)
        side = np.zeros((n, 8), np.float32)
        side[:, 0] = np.where(rng.random(n) < 0.5, -half, -half - 1.0)
        side[:, 1] = rng.choice([0.0, -0.0, 0.0625, -1e-7], n)
        side[:, 2] = rng.integers(-q // 2, q // 2 + 1, n) * step
        side[:, 3] = 1.0; side[:, 4] = rng.choice([0.0, -0.0], n); side[:, 5] = rng.choice([0.0, -0.0], n)
        side[:, 7] = 1e30
        sw = rng.random(n) < 0.5                                          # half of them along z instead
        side[sw] = side[sw][:, [2, 1, 0, 5, 4, 3, 6, 7]]
        s.compare(side, "grid: along x / z")
        # in the grid's plane, in arbitrary directions
        ang = rng.uniform(0, 2 * np.pi, n)
        plane = np.zeros((n, 8), np.float32)
        plane[:, 0], plane[:, 2] = rng.uniform(-half, half, n), rng.uniform(-half, half, n)
        plane[:, 3], plane[:, 5] = np.cos(ang), np.sin(ang)
        plane[:, 7] = 1e30
        s.compare(plane, "grid: in the plane")
    finally:
        s.close()


def test_collinear_slivers(built):
    rng = np.random.default_rng(12)
    n = 1500
    a = rng.uniform(-1, 1, (n, 3)); d = rng.normal(0, 0.2, (n, 3))
    slivers = np.stack([a, a + d, a + rng.choice([0.5, 2.0, -1.0], n)[:, None] * d], 1).astype(np.float32)
    s = Scene(SMALL0, mesh_from_tris(np.concatenate([slivers, soup(500, seed=13)])))
    try:
        lo, hi = model_box(s)
        rays = rays_through_box(lo, hi, 2500, seed=14)
        along = rays[:500].copy()                                         # aimed along a sliver's line, from beyond its end
        k = rng.integers(0, n, 500)
        along[:, :3] = slivers[k, 0] - 3.0 * (slivers[k, 1] - slivers[k, 0]); along[:, 3:6] = slivers[k, 1] - slivers[k, 0]
        s.compare(np.concatenate([rays, along]), "slivers", min_hits=1)
    finally:
        s.close()


def test_one_huge_triangle_among_thousands_in_one_morton_cell(built):
    """The Morton box is the vertex bounds: with one triangle 1e6 wide, 4000 tiny ones a thousandth across share one cell."""
    tiny = soup(4000, seed=15, extent=1e-3, size=1e-4)
    huge = np.array([[[-1e6, -1e-3, -1e6], [1e6, -2e-3, -1e6], [0.0, 2e-3, 1e6]]], np.float32)
    s = Scene(SMALL0, mesh_from_tris(np.concatenate([tiny[:2000], huge, tiny[2000:]])), world0=world(1.0, (0.0, 1e7, 0.0)))
    try:
        s.compare(rays_through_box((-1e-3,) * 3, (1e-3,) * 3, 3000, seed=16), "huge + tiny", min_hits=1000)
    finally:
        s.close()


def test_same_mesh_in_both_slots_ties_go_to_instance_zero(built):
    m = mesh_from_tris(soup(2000, seed=17))
    w = world(1.0, (0.5, 0.25, 0.0))
    s = Scene(m, m, world0=w, world1=w)
    try:
        lo, hi = model_box(s)
        b = s.compare(rays_through_box(lo, hi, 3000, seed=18), "same mesh twice", min_hits=500)
        assert (b["inst"][b["valid"]] == 0).all()
    finally:
        s.close()


# ---- a traversal stack deeper than the LDS part ----------------------------------------------------------------------------------
def telescope(copies=100, s=0.9):
    """Copies of one triangle, each s times the size of the one before and moved toward -z by half the room that leaves: every
    copy's box lies strictly inside the box of every larger copy.  Merged with anything smaller, a copy's box is its own: PLOC can
    only add the next copy to the cluster of the smaller ones, whatever its tie rule -- a caterpillar `copies` levels deep.  Primitive 0
    is the smallest copy (equal Morton codes keep the order of size, so that the cluster is always the left child)."""
    base = np.array([[-1.0, -1.0, -1.0], [1.0, -1.0, 0.0], [0.0, 1.0, 1.0]])
    tris, zc = [], 0.0
    for k in range(copies):
        tris.append(base * s ** k + np.array([0.0, 0.0, zc]))
        zc -= 0.5 * s ** k * (1.0 - s)
    return np.array(tris[::-1], np.float32), np.float32(zc + 0.5 * s ** (copies - 1) * (1.0 - s))


def deepest_push_before_first_leaf(nodes4_u32, root, rays):
    """Replay of the trace kernel's 4-wide step (csrc/trace.hip, node phase: entry distances by the slab test, misses at infinity,
    the same five compare-exchanges, the first entry taken, the other hits pushed from the last) from the root until the first leaf:
    the stack a lane holds at that point.  Until then no triangle has been tested, so tmax bounds the boxes.  Used on rays that start
    strictly inside every box (entry distance = tmin for all of them, whatever the rounding), so the replay is exact."""
    nodes4 = nodes4_u32.reshape(-1, 32)
    f = nodes4[:, :24].view(np.float32).astype(np.float64).reshape(-1, 6, 4)
    ref = nodes4[:, 24:28].view(np.int32)
    deepest = []
    for r in rays.astype(np.float64):
        o, d, tmin, tmax = r[:3], r[3:6], r[6], r[7]
        cur, sp = root, 0
        while cur >= 0:
            lo, hi = f[cur, :3].T, f[cur, 3:].T                           # [4 entries, 3]
            assert ((lo < o) & (o < hi) | (ref[cur] == EMPTY)[:, None]).all(), "the replay needs origins inside every box"
            with np.errstate(divide="ignore"):
                far = np.where(d != 0, np.maximum((lo - o) / d, (hi - o) / d), np.inf).min(axis=1)
            t = [tmin if (ref[cur][e] != EMPTY and tmin <= min(far[e], tmax)) else np.inf for e in range(4)]
            c = [int(x) for x in ref[cur]]
            for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):        # RT_CSWAP: exchange only when strictly smaller
                if t[b] < t[a]:
                    t[a], t[b], c[a], c[b] = t[b], t[a], c[b], c[a]
            assert t[0] < np.inf, "a ray of the replay leaves the tree before a leaf"
            sp += sum(1 for e in (1, 2, 3) if t[e] < np.inf)
            cur = c[0]
        deepest.append(sp)
    return np.array(deepest)


def test_telescope_spills_the_traversal_stack(built):
    """RT_STACK = 16 entries of the stack live in LDS, the rest in global memory (trace.hip RT_PUSH / popOrFinish), sized from the
    build's BuildResult::stack4.  Rays from inside the smallest copy of the telescope enter every box at tmin: the kernel's stable
    exchanges keep the entries in order, the nested subtree first, and each 4-wide level pushes the other three."""
    tris, inner = telescope()
    n = len(tris)
    s = Scene(SMALL0, mesh_from_tris(tris), world0=world(1.0, (0.0, 50.0, 0.0)))
    try:
        assert n <= s.depth[1] <= 128, "the telescope is a caterpillar: depth %d" % s.depth[1]
        rng = np.random.default_rng(19)
        m = 2000
        inside = np.zeros((m, 8), np.float32)                             # from the smallest copy's centre, in every direction
        inside[:, 2] = inner
        d = rng.normal(size=(m, 3)); inside[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
        inside[:m // 4, 3:6] = [0.0, 0.0, 1.0]                            # (and straight up the axis: through every copy)
        inside[:, 7] = 1e30
        deepest = deepest_push_before_first_leaf(s.ctx.readback(s.capi.BUF_BVH4_NODES1), s.ctx.bvh_root(1), inside[:: m // 64])
        assert deepest.min() > RT_STACK, "the replayed stack holds %d entries: the spill path was not reached" % deepest.min()
        b = s.compare(inside, "telescope, from inside", min_hits=m // 4)
        assert (b["prim"][:m // 4] == 0).all() and (b["inst"][:m // 4] == 1).all(), "up the axis the smallest copy is the nearest"
        s.compare(rays_through_box(tris.min(axis=(0, 1)), tris.max(axis=(0, 1)), 2000, seed=20), "telescope, random", min_hits=500)
    finally:
        s.close()
