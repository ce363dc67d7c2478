"""The sun on the GPU (rtggx_set_sun; lighting.hip sunGenKernel, the any-hit traversal, sunAddKernel): frames bit for bit against the
restatement (tests/sun_ref.cpp) behind the depth, sample-count, sampler and sample-set restatements; all-metal carry-over; a 1080p frame; the
sun turned off again against a twin; still sky; refusals; strips; accumulation.  Direction and irradiance are those of
tests/golden/sun_classes.json, whose class shares tests/test_sun_host.py establishes on the CPU."""
import json
import os

import numpy as np
import pytest

import accum_ref as AR
import gpu_support as G
import sun_ref as SR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sun_classes.json")))
L, E = GOLDEN["direction"], GOLDEN["irradiance"]
MIXED = tuple(GOLDEN["metallic"])
SUN_ARGS = ["-sun"] + [str(x) for x in L + E]
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS


def sun_pair(W, H, metallic=MIXED, depth=1, samples=1, sample_set=256, vndf=False):
    """gpu_support.restated_pair with the sun's oracle, both sides lit."""
    p = G.Pair(W, H, metallic=metallic, oracle=lambda w, h: SR.Oracle(w, h, depth=depth, samples=samples, sample_set=sample_set))
    p.ctx.set_sample_set(sample_set)
    if samples != 1:
        p.ctx.set_samples_per_pixel(samples)
    if depth != 1:
        p.ctx.set_max_recursion_depth(depth)
    if vndf:
        p.ctx.set_sampler(True); p.o.set_sampler(True)
    p.ctx.set_sun(L, E); p.o.set_sun(L, E)
    return p


def class_counts(classes):
    return [int((classes == k).sum()) for k in (SR.FACING_AWAY, SR.OCCLUDED, SR.LIT)]


@pytest.mark.parametrize("setting", [dict(), dict(depth=2), dict(samples=2), dict(vndf=True), dict(sample_set=1024)],
                         ids=["depth 1", "depth 2", "N = 2", "VNDF", "M = 1024"])
def test_frames_equal_the_restatement(built, setting):
    """100 x 54 bunny, both images take part, three frames: G-buffer, RayTracingOut0/1 and the ray count bit for bit / equal, the denoised
    images under the existing bars.  Every covered class holds a twentieth of the covered pixels (the golden file's bar) in every frame."""
    p = sun_pair(GOLDEN["width"], GOLDEN["height"], **setting)
    try:
        for f in range(3):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            p.check_frame("frame %d" % f)
            counts = class_counts(p.o.classes)
            assert min(counts) >= 0.05 * sum(counts), counts
    finally:
        p.close()


def test_all_metal_the_carry_over_stays(built):
    """Default materials: RayTracingOut1 is carried over and the sun does not touch it -- equal to the restatement's, and to a sunless twin's."""
    p, b = sun_pair(100, 54, metallic=None), G.app(100, 54)
    try:
        for f in range(3):
            p.frame(); G.frame(b)
            G.check_raw(p, "frame %d" % f, require_rays=True)
            ib = G.images(b, ("diff", "refl"))
            np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), ib["diff"], err_msg="frame %d: RayTracingOut1" % f)
            assert (p.ctx.readback(p.capi.BUF_RT_REFL) != ib["refl"]).any()
    finally:
        p.close(); b.OnDestroy()


def test_a_1080p_frame_equals_the_restatement(built):
    """The shadow launch in the frame's resident-workgroup shape (some 6 x 10^5 shadow rays)."""
    p = sun_pair(1920, 1080)
    try:
        for f in range(2):      # (the second frame's launch shapes follow the first frame's ray count)
            p.frame()
        G.check_raw(p, "1080p", require_rays=True)
        assert sum(class_counts(p.o.classes)[1:]) >= 200000
    finally:
        p.close()


def test_the_sun_turned_off_again_leaves_a_default_context(built):
    a, b = G.app(320, 180, ["-metallic", MIXED[0], MIXED[1]]), G.app(320, 180, ["-metallic", MIXED[0], MIXED[1]])
    try:
        a.context.set_sun(L, E)
        for f in range(3):
            G.frame(a); G.frame(b)
            ia, ib = G.images(a, IMAGES), G.images(b, IMAGES)
            assert ia["rays"][0] > ib["rays"][0] and (ia["refl"] != ib["refl"]).any() and (ia["diff"] != ib["diff"]).any()
            G.assert_same({k: ia[k] for k in G.GBUFFER}, {k: ib[k] for k in G.GBUFFER}, "lit frame %d" % f)
        a.context.set_sun(None, None)
        for f in range(6):      # (the temporal history forgets the lit frames geometrically: the raw images and the rays are equal at once)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, G.GBUFFER + G.RAW + G.RAYS), G.images(b, G.GBUFFER + G.RAW + G.RAYS), "dark frame %d" % f)
            assert a.context.placement()[0] == b.context.placement()[0]
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_a_context_that_had_a_sun_before_its_first_frame_equals_one_that_never_had(built):
    """Every buffer through the back buffer: the twin launches the default kernels only (ray count, placement)."""
    a, b = G.app(320, 180), G.app(320, 180)
    try:
        a.context.set_sun(L, E); a.context.set_sun(L, (0.0, 0.0, 0.0))
        for f in range(3):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
            assert a.context.placement() == b.context.placement()
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_still_sky_runs_go_on_across_set_sun(built):
    """A still camera: the runs of the tiles nothing is drawn in keep growing across the call, and the images equal those of a context that leaves no tile alone."""
    a, b = G.app(320, 180), G.app(320, 180)
    try:
        b.context.static_sky(False)
        before = None
        for f in range(20):
            if f == 14:
                before = a.context.sky_runs()[0].copy()
                a.context.set_sun(L, E); b.context.set_sun(L, E)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
        runs, threshold = a.context.sky_runs()
        assert (before >= threshold).any() and (runs[before >= threshold] > before[before >= threshold]).all()
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_refusals_leave_the_context_as_it_was(built):
    from raytracedggx_amd import capi
    a, b = G.app(100, 54), G.app(100, 54)
    try:
        a.context.set_ray_rate(4)
        with pytest.raises(capi.RtggxError, match="rtggx_set_sun"):
            a.context.set_sun(L, E)
        a.context.set_ray_rate(1)
        for bad in ((0.0, 0.0, 0.0), (float("nan"), 1.0, 0.0), (float("inf"), 1.0, 0.0)):
            with pytest.raises(capi.RtggxError, match="rtggx_set_sun"):
                a.context.set_sun(bad, E)
        with pytest.raises(capi.RtggxError, match="rtggx_set_sun"):
            a.context.set_sun(L, (1.0, -1.0, 1.0))
        G.frame(a); G.frame(b)
        G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "after the refusals")
        a.context.set_sun(L, E); b.context.set_sun(L, E)
        with pytest.raises(capi.RtggxError, match="rtggx_set_ray_rate"):
            a.context.set_ray_rate(4)
        G.frame(a); G.frame(b)
        G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "rate 4 refused on a lit context")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_strips_equal_the_full_frame(built):
    assert G.strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=tuple(SUN_ARGS) + ("-metallic", str(MIXED[0]), str(MIXED[1]))) > 0


def test_accumulated_sums_equal_the_restatement_fed_the_lit_words(built):
    from raytracedggx_amd import capi
    a = G.app(100, 54, ["-metallic", MIXED[0], MIXED[1]] + SUN_ARGS)
    try:
        a.context.set_accumulation(True)
        acc = AR.Accumulator(54, 100)
        for f in range(4):
            G.frame(a)
            c = a.context
            c.sync()
            acc.add(c.readback(capi.BUF_RT_REFL), c.readback(capi.BUF_RT_DIFF), c.readback(capi.BUF_VISIBILITY), MIXED)
            assert c.accumulated_frames() == acc.frames
            for got, want in ((c.readback(capi.BUF_ACC_REFL), acc.refl), (c.readback(capi.BUF_ACC_DIFF), acc.diff)):
                assert AR.same_bits(got, want).all(), "frame %d" % f
    finally:
        a.OnDestroy()


def test_a_score_record_equals_the_restatement_on_the_lit_words(built):
    """The reference is the lit frame's own first TemporalSSOut: any RGBA16F image serves, the record is what is compared."""
    import score_ref
    from raytracedggx_amd import capi
    a = G.app(100, 54, ["-metallic", MIXED[0], MIXED[1]] + SUN_ARGS)
    try:
        c = a.context
        G.frame(a); c.sync()
        ref = c.readback(capi.BUF_TSS0 + c.frame_parity())
        c.set_reference(ref); c.set_scoring(True)
        for f in range(2):
            G.frame(a); c.sync()
            words = (c.readback(capi.BUF_TSS0 + c.frame_parity()), c.readback(capi.BUF_RT_REFL), c.readback(capi.BUF_RT_DIFF), c.readback(capi.BUF_VISIBILITY))
            recs = c.read_scores()
            assert len(recs) == 1
            want = score_ref.score(words[0], words[1], words[2], words[3], MIXED, ref, 0, None)
            bad = score_ref.same_record(recs[0], want)
            assert not bad, "frame %d: %s differ" % (f, bad)
            assert want["se_raw_rgb"] > 0.0
    finally:
        a.OnDestroy()


def test_a_deforming_mesh_moves_its_shadow(built):
    """gpu_support.wave, three frames: each frame equals the restatement on the moved mesh and the refitted tree, and the set of occluded
    pixels changes with the shape."""
    import assets
    p = sun_pair(320, 180)
    try:
        p.frame(); G.check_raw(p, "before the deformation", require_rays=True)
        v0, idx, _ = O.obj_import(assets.path("bunny.obj"))
        shadows = [p.o.classes == SR.OCCLUDED]
        for f in range(1, 4):
            v = G.wave(v0, f)
            p.ctx.refit_as(1, v)
            p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
            p.o.set_mesh(1, v, idx)
            p.give_oracle_the_device_trees(refitted=True)
            p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
            p.o.update_as(); p.o.render_visibility(); p.rays = p.o.ray_trace()
            G.check_raw(p, "deformed, frame %d" % f, require_rays=True)
            shadows.append(p.o.classes == SR.OCCLUDED)
            assert shadows[-1].any() and (shadows[-1] != shadows[-2]).any()
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()
