"""Occlusion queries (rtggx_trace_occlusion): the any-hit variant of the trace kernel (csrc/trace.hip traceKernel<.., ANY = true>; the
contract is in csrc/rt_queue.h) on the synthetic meshes the closest-hit traversal is tested on.

The tested equality, for every ray:  trace_occlusion(rays) == trace_rays(rays)["valid"] == the oracle's brute-force loop over all
triangles.  An occluded ray says nothing else -- which triangle stopped it is unspecified --, so there is nothing to compare beyond
that bit; what can go wrong is the bit itself: a job that leaves at its first triangle and drops its stack (LDS and spilled), helpers
that took subtrees of a ray somebody else then finds occluded, a primary job that skips the second instance, both bounds of the
interval, and every launch shape (single-wave workgroups, which every list launches; resident workgroups, through a child process with
RTGGX_TRACE_WAVES set; one, two and eight waves per bin; several launches where a list exceeds the bins)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_support as G
import occlusion_cases as OC
from bvh_cases import grid_mesh, mesh_from_tris, rays_through_box, soup, world
from gpu_support import Scene, model_box
from occlusion_cases import SMALL0, telescope

pytestmark = pytest.mark.gpu


def occlusion_equals_valid(s, rays, label, min_hits=1, min_misses=1):
    """trace_occlusion == the closest-hit kernel's valid == brute force, ray by ray; returns the brute-force record."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    occ = s.ctx.trace_occlusion(rays)
    assert occ.dtype == np.bool_ and occ.shape == (len(rays),)
    g = s.ctx.trace_rays(rays)["valid"]
    b = s.o.trace_rays(rays, brute=True)
    for other, what in ((g, "the closest-hit kernel"), (b["valid"], "brute force")):
        bad = np.nonzero(occ != other)[0]
        assert bad.size == 0, "%s: %d of %d rays differ from %s, first ray %d: %s, occluded %s" % (
            label, bad.size, len(rays), what, bad[0], rays[bad[0]].tolist(), bool(occ[bad[0]]))
    assert b["valid"].sum() >= min_hits and (~b["valid"]).sum() >= min_misses, "%s: %d of %d rays hit" % (label, b["valid"].sum(), len(rays))
    return b


def interval_edges(s, rays, label):
    """gpu_support.interval_edges for the one bit: both bounds are exclusive, so with tmax (or tmin) at the exact t of the closest hit
    that hit must go -- the ray stays occluded only by what lies strictly inside --, and an empty interval is never occluded."""
    b = s.o.trace_rays(rays, brute=True)
    hit, t = rays[b["valid"]].copy(), b["t"][b["valid"]]
    assert hit.shape[0] > 0, label
    at_tmax = hit.copy(); at_tmax[:, 7] = t
    e = occlusion_equals_valid(s, at_tmax, label + ", tmax = t of the closest hit", 0, 1)
    assert not e["valid"].all(), label + ": nothing went with tmax = t"
    at_tmin = hit.copy(); at_tmin[:, 6] = t
    occlusion_equals_valid(s, at_tmin, label + ", tmin = t of the closest hit", 0, 0)
    empty = hit.copy(); empty[:, 6] = t; empty[:, 7] = t
    assert not s.ctx.trace_occlusion(empty).any(), label + ": an empty interval is occluded"
    rev = hit.copy(); rev[:, 6] = t; rev[:, 7] = t * np.float32(0.5)
    assert not s.ctx.trace_occlusion(rev).any(), label + ": tmin > tmax is occluded"


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 1025, 40000])
def test_random_soup_in_the_model_slot(built, n):
    s = Scene(SMALL0, mesh_from_tris(soup(n, seed=n)), world1=world(1.0, (0.25, 0.5, -0.125), rot_y90=(n % 2 == 1)))
    try:
        lo, hi = model_box(s)
        rays = rays_through_box(lo, hi, 3000 if n < 10000 else 1500, seed=n)
        occlusion_equals_valid(s, rays, "soup of %d" % n)
        interval_edges(s, rays[:500], "soup of %d" % n)
    finally:
        s.close()


@pytest.mark.parametrize("n", [2, 97, 3073])
def test_random_soup_in_the_ground_slot(built, n):
    """Both instances overlap: a ray occluded in instance 0 does not enter instance 1, one that is not must still be tested there."""
    s = Scene(mesh_from_tris(soup(n, seed=1000 + n)), mesh_from_tris(soup(300, seed=7)),
              world0=world(2.0, (0.5, 0.0, 0.0)), world1=world(1.0, (0.0, 0.0, 0.5)))
    try:
        lo, hi = model_box(s, 0)
        rays = rays_through_box(lo, hi, 3000, seed=n)
        b = occlusion_equals_valid(s, rays, "ground soup of %d" % n)
        assert (b["inst"][b["valid"]] == 1).any(), "no ray is occluded by the model alone"
    finally:
        s.close()


def test_coincident_triangles(built):
    """3000 copies of one triangle: every job of an occluded ray meets a triangle it accepts."""
    tri = np.array([[-1.0, -0.5, 0.25], [1.0, -0.25, -0.25], [0.125, 1.0, 0.0]], np.float32)
    s = Scene(SMALL0, mesh_from_tris(np.repeat(tri[None], 3000, axis=0)))
    try:
        rays = rays_through_box(tri.min(axis=0), tri.max(axis=0), 3000, seed=3)
        occlusion_equals_valid(s, rays, "coincident", min_hits=500)
        interval_edges(s, rays[:300], "coincident")
    finally:
        s.close()


def test_every_triangle_twice_with_reversed_winding(built):
    """The same triangle wound both ways: t may differ in its last bit between the two, so with tmax at the closest t the twin decides."""
    t = soup(1500, seed=8)
    s = Scene(SMALL0, mesh_from_tris(np.concatenate([t, t[:, [0, 2, 1]]])))
    try:
        lo, hi = model_box(s)
        rays = rays_through_box(lo, hi, 3000, seed=9)
        occlusion_equals_valid(s, rays, "reversed winding", min_hits=300)
        interval_edges(s, rays[:500], "reversed winding")
    finally:
        s.close()


def test_same_mesh_in_both_slots(built):
    m = mesh_from_tris(soup(2000, seed=17))
    w = world(1.0, (0.5, 0.25, 0.0))
    s = Scene(m, m, world0=w, world1=w)
    try:
        lo, hi = model_box(s)
        rays = rays_through_box(lo, hi, 3000, seed=18)
        occlusion_equals_valid(s, rays, "same mesh twice", min_hits=500)
        interval_edges(s, rays[:300], "same mesh twice")
    finally:
        s.close()


def test_flat_grid_and_axis_aligned_rays_along_shared_edges(built):
    q, step = 128, 0.125
    v, idx = grid_mesh(q, step)
    s = Scene(SMALL0, (v, idx), world0=world(1.0, (0.0, 100.0, 0.0)))      # (the ground's soup out of the way, above)
    try:
        rng = np.random.default_rng(10)
        half = q / 2 * step
        occlusion_equals_valid(s, rays_through_box((-half, -0.5, -half), (half, 0.5, half), 3000, seed=11), "grid: random", min_hits=500, min_misses=0)
        # straight down / up through vertices, edges and quads, with -0.0 direction components
        n = 1200
        xz = np.stack([rng.integers(-q // 2, q // 2 + 1, n) * step / rng.choice([1, 2, 4], n),
                       rng.integers(-q // 2, q // 2 + 1, n) * step / rng.choice([1, 2, 4], n)], 1).astype(np.float32)
        y0 = rng.choice([1.0, 0.125, -2.0], n).astype(np.float32)
        down = np.zeros((n, 8), np.float32)
        down[:, 0], down[:, 1], down[:, 2] = xz[:, 0], y0, xz[:, 1]
        down[:, 3] = np.where(rng.random(n) < 0.5, -0.0, 0.0); down[:, 5] = np.where(rng.random(n) < 0.5, -0.0, 0.0)
        down[:, 4] = np.where(y0 > 0, -1.0, 1.0)
        down[:, 7] = 1e30
        occlusion_equals_valid(s, down, "grid: axis-aligned", min_hits=n // 2, min_misses=0)
        interval_edges(s, down[:300], "grid: axis-aligned")
        # along x and z in or beside the grid's plane, along its shared edges
        side = np.zeros((n, 8), np.float32)
        side[:, 0] = np.where(rng.random(n) < 0.5, -half, -half - 1.0)
        side[:, 1] = rng.choice([0.0, -0.0, 0.0625, -1e-7], n)
        side[:, 2] = rng.integers(-q // 2, q // 2 + 1, n) * step
        side[:, 3] = 1.0; side[:, 4] = rng.choice([0.0, -0.0], n); side[:, 5] = rng.choice([0.0, -0.0], n)
        side[:, 7] = 1e30
        sw = rng.random(n) < 0.5                                          # half of them along z instead
        side[sw] = side[sw][:, [2, 1, 0, 5, 4, 3, 6, 7]]
        occlusion_equals_valid(s, side, "grid: along x / z", min_hits=0, min_misses=0)
    finally:
        s.close()


def test_telescope_a_spilled_stack_is_dropped_or_drained(built):
    """The telescope's traversal stack spills to global memory (tests/test_gpu_bvh_meshes.py shows that it does, for these very rays).
    From inside the smallest copy: up the axis every copy is hit -- the job leaves with most of its spilled stack unread --, in other
    directions the rays leave through some of the copies or none, and a ray that hits nothing has to drain all of it."""
    tris, inner = telescope()
    s = Scene(SMALL0, mesh_from_tris(tris), world0=world(1.0, (0.0, 50.0, 0.0)))
    try:
        rng = np.random.default_rng(19)
        m = 2000
        inside = np.zeros((m, 8), np.float32)
        inside[:, 2] = inner
        d = rng.normal(size=(m, 3)); inside[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
        inside[:m // 4, 3:6] = [0.0, 0.0, 1.0]
        inside[:, 7] = 1e30
        b = occlusion_equals_valid(s, inside, "telescope, from inside", min_hits=m // 4)
        assert b["valid"][:m // 4].all()
        interval_edges(s, inside[:600], "telescope, from inside")
        occlusion_equals_valid(s, rays_through_box(tris.min(axis=(0, 1)), tris.max(axis=(0, 1)), 2000, seed=20), "telescope, random", min_hits=500)
    finally:
        s.close()


# ---- list lengths and launch shapes -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soup_scene(built):
    s = Scene(mesh_from_tris(soup(97, seed=1097)), mesh_from_tris(soup(5000, seed=21)), world0=world(2.0, (0.5, 0.0, 0.0)), world1=world(1.0, (0.0, 0.0, 0.5)))
    yield s
    s.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4097])
def test_short_lists(soup_scene, n):
    """Around a wave, a bin (64 slots) and the bins of the 64 x 64 context (4096 slots: the 4097th ray is a second launch)."""
    s = soup_scene
    lo, hi = model_box(s)
    rays = rays_through_box(lo, hi, 4097, seed=22)[:n]
    occlusion_equals_valid(s, rays, "%d rays" % n, min_hits=0, min_misses=0)
    np.testing.assert_array_equal(s.ctx.trace_occlusion(rays), s.ctx.trace_occlusion(rays), err_msg="a repeated call")


@pytest.fixture(scope="module")
def long_lists(built):
    ctx, o, rays = OC.long_list_context()
    yield ctx, o, rays
    ctx.close(); o.close()


@pytest.mark.parametrize("n", [30000, 100000, 262144])
def test_long_lists(long_lists, n):
    """One launch each (the context's bins hold 524 288 rays).  A list is alone on the chip and launches single-wave workgroups whatever its
    length: eight, two and one wave per bin here (chooseSliceShift)."""
    OC.check_long_list(*long_lists, n)


def test_resident_workgroups_through_the_forced_size(built):
    """The resident shape of the variant -- one workgroup of 12 waves per CU with the tree tops in LDS, what a launch inside a frame has from
    RT_TINY_RAYS rays on -- is reached by a list only through RTGGX_TRACE_WAVES, read once per process: hence a child."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "occlusion_forced_child.py")], env=dict(os.environ, RTGGX_TRACE_WAVES="12"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "resident lists ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_refusals(soup_scene):
    from raytracedggx_amd import capi
    s = soup_scene
    L = capi.load()
    out = np.zeros(4, np.uint32)
    rays = np.zeros((4, 8), np.float32)
    assert L.rtggx_trace_occlusion(s.ctx.h, rays.ctypes.data, 0, out.ctypes.data) != 0, "n == 0"
    assert L.rtggx_trace_occlusion(s.ctx.h, None, 4, out.ctypes.data) != 0, "null rays"
    assert L.rtggx_trace_occlusion(s.ctx.h, rays.ctypes.data, 4, None) != 0, "null result"
    fresh = capi.Context(64, 64)
    try:
        with pytest.raises(capi.RtggxError, match="rtggx_trace_occlusion"):
            fresh.trace_occlusion(rays)      # before rtggx_build_as
    finally:
        fresh.close()


# ---- between frames ---------------------------------------------------------------------------------------------------------------
def test_a_call_between_frames_leaves_the_next_frames_as_they_were(built):
    """The call refills a set's ray bins (and ends the still-sky runs for it): the frames after it equal those of a twin context that
    made no such call, in every buffer and in the ray count."""
    a, b = G.app(320, 180), G.app(320, 180)
    try:
        rays = rays_through_box((-8, -2, -8), (8, 8, 8), 5000, seed=24)
        for f in range(4):
            G.frame(a); G.frame(b)
            what = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
            G.assert_same(G.images(a, what), G.images(b, what), "frame %d" % f)
            if f in (0, 1):
                occ = a.context.trace_occlusion(rays)
                np.testing.assert_array_equal(occ, a.context.trace_rays(rays)["valid"])
                assert occ.any() and not occ.all()
    finally:
        a.OnDestroy(); b.OnDestroy()
