"""The sun at the surfaces the paths hit, on the GPU (rtggx_set_sun_reflections; lighting.hip sunHitGenKernel, the any-hit traversal,
sunHitAddKernel, sunHitResolveKernel): frames bit for bit against the restatement (tests/sun_hit_ref.cpp) at every depth, with several
samples, a sample map, the other sampler and a larger sample set; both bin sizes; preset returns; a 1080p frame; twins; refusals; strips;
accumulation and scoring; a deforming mesh; still sky.  Scene, direction and irradiance are those of tests/golden/sun_hit_classes.json,
whose class shares tests/test_sun_hit_host.py establishes on the CPU."""
import json
import os

import numpy as np
import pytest

import accum_ref as AR
import adaptive_ref as AD
import gpu_support as G
import sun_hit_ref as SH
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sun_hit_classes.json")))
L, E = GOLDEN["direction"], GOLDEN["irradiance"]
W, H = GOLDEN["width"], GOLDEN["height"]      # 148 x 84: ragged right and bottom edges (no multiple of 8 or 16), 10 x 6 tiles
MIXED = tuple(GOLDEN["metallic"])
SUN_ARGS = ["-sun"] + [str(x) for x in L + E]
METAL_ARGS = ["-metallic", str(MIXED[0]), str(MIXED[1])]
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS


def hit_pair(width, height, metallic=MIXED, depth=1, samples=1, sample_set=256, vndf=False):
    """gpu_support.restated_pair with this feature's oracle, both sides lit and with the toggle on."""
    p = G.Pair(width, height, metallic=metallic, oracle=lambda w, h: SH.Oracle(w, h, depth=depth, samples=samples, sample_set=sample_set))
    p.ctx.set_sample_set(sample_set)
    if samples != 1:
        p.ctx.set_samples_per_pixel(samples)
    if depth != 1:
        p.ctx.set_max_recursion_depth(depth)
    if vndf:
        p.ctx.set_sampler(True); p.o.set_sampler(True)
    p.ctx.set_sun(L, E); p.o.set_sun(L, E)
    p.ctx.set_sun_reflections(1); p.o.set_sun_reflections(True)
    return p


def assert_class_conditions(o, depth, label):
    """The golden file's conditions on the frame the oracle has just traced."""
    level0 = [o.count(k, 0) for k in SH.CLASSES]
    assert min(level0) >= 0.05 * sum(level0), (label, level0)
    if depth >= 2:
        level1 = [o.count(k, 1) for k in SH.CLASSES]
        assert min(level1) >= 20, (label, level1)
    assert o.count("specular") > 0 and o.count("diffuse") > 0, label


SETTINGS = [dict(), dict(depth=2), dict(depth=3), dict(samples=2), dict(samples=4, mapped=True), dict(vndf=True), dict(sample_set=1024)]


@pytest.mark.parametrize("setting", SETTINGS, ids=["depth 1", "depth 2", "depth 3", "N = 2", "N = 4 mapped 1 2 4", "VNDF", "M = 1024"])
def test_frames_equal_the_restatement(built, setting):
    """148 x 84 bunny, metallic (0.25, 0.75) -- 128-slot bins in two compaction rounds, both lobes, ragged edges --, three frames: G-buffer,
    RayTracingOut0/1 and the ray count bit for bit / equal, the denoised images under the existing bars, the class conditions in every frame."""
    setting = dict(setting)
    mapped = setting.pop("mapped", False)
    p = hit_pair(W, H, **setting)
    try:
        blocks = None
        if mapped:
            by, bx = AD.blocks_of(W, H)
            y, x = np.mgrid[0:by, 0:bx]
            blocks = np.array([1, 2, 4], np.uint8)[(x + 2 * y) % 3]
            p.ctx.set_sample_map(blocks)
        for f in range(3):
            label = "frame %d" % f
            if mapped:
                p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
                p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
                p.o.update_as(); p.o.render_visibility()
                p.rays = SH.mapped_frame(p.o, blocks)
                p.o.denoise(); p.o.tone_map()
            else:
                p.frame()
            G.check_raw(p, label, require_rays=True)
            p.check_frame(label)
            assert p.o.hit_rays > 0
            assert_class_conditions(p.o, setting.get("depth", 1), label)
    finally:
        p.close()


def test_all_metal_64_slot_bins_and_the_carry_over(built):
    """Default materials: bins of 64 slots, no diffuse path -- RayTracingOut1 equals the restatement's and a sunless twin's."""
    p, b = hit_pair(W, H, metallic=None, depth=2), G.app(W, H, ["-recursion", "2"])
    try:
        for f in range(3):
            p.frame(); G.frame(b)
            G.check_raw(p, "frame %d" % f, require_rays=True)
            ib = G.images(b, ("diff", "refl"))
            np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), ib["diff"], err_msg="frame %d: RayTracingOut1" % f)
            assert (p.ctx.readback(p.capi.BUF_RT_REFL) != ib["refl"]).any()
            assert p.o.count("lit", 0) > 0 and p.o.count("lit", 1) > 0 and p.o.count("diffuse") == 0 and not (p.o.lit & 2).any()
    finally:
        p.close(); b.OnDestroy()


def test_preset_returns_trace_no_shadow_ray(built):
    """Metallic (0.0, 1.0): the ground's reflection rays return their preset without looking at the surface they hit -- no term, and no
    shadow ray (the ray count is the restatement's)."""
    p = hit_pair(W, H, metallic=(0.0, 1.0), depth=2)
    try:
        for f in range(2):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            assert p.o.count("preset") > 0 and p.o.hit_rays > 0
    finally:
        p.close()


@pytest.mark.parametrize("samples", [2, 1], ids=["N = 2", "N = 1"])
def test_a_1080p_frame_equals_the_restatement(built, samples):
    """The second of two frames at depth 2: the resident launch shape, the main stream and its spill part.  Two samples: the terms in the
    sample sums, at least 2 x 10^5 shadow rays from hits (one sample has 1.35 x 10^5 at depth 1 and 1.8 x 10^5 at depth 2: below the bar,
    so the bar is asserted here); one sample: S and its resolve at full size."""
    p = hit_pair(1920, 1080, depth=2, samples=samples)
    try:
        for f in range(2):
            p.frame()
        G.check_raw(p, "1080p", require_rays=True)
        assert p.o.hit_rays >= (200000 if samples == 2 else 1), p.o.hit_rays
        key, where = p.ctx.placement()
        assert not key["small"] and where["shade"] == "main", (key, where)
    finally:
        p.close()


def twins(a, b, frames, label, denoised=True):
    for f in range(frames):
        G.frame(a); G.frame(b)
        names = IMAGES if denoised else G.GBUFFER + G.RAW + G.RAYS
        G.assert_same(G.images(a, names), G.images(b, names), "%s, frame %d" % (label, f))
        assert a.context.placement() == b.context.placement(), "%s, frame %d: placement" % (label, f)


def test_the_toggle_without_a_sun_is_a_default_context(built):
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        a.context.set_sun_reflections(1)
        twins(a, b, 3, "toggle on, no sun")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_the_toggle_turned_off_again_is_the_sun_alone(built):
    a, b = G.app(320, 180, METAL_ARGS + SUN_ARGS), G.app(320, 180, METAL_ARGS + SUN_ARGS)
    try:
        a.context.set_sun_reflections(1)
        for f in range(3):
            G.frame(a); G.frame(b)
            ia, ib = G.images(a, IMAGES), G.images(b, IMAGES)
            assert ia["rays"][0] > ib["rays"][0] and (ia["refl"] != ib["refl"]).any() and (ia["diff"] != ib["diff"]).any()
            G.assert_same({k: ia[k] for k in G.GBUFFER}, {k: ib[k] for k in G.GBUFFER}, "toggle on, frame %d" % f)
        a.context.set_sun_reflections(0)
        twins(a, b, 6, "toggle off again", denoised=False)      # (the temporal history forgets the earlier frames geometrically)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_the_toggle_set_before_the_first_frame_with_the_sun_turned_off(built):
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        a.context.set_sun(L, E); a.context.set_sun_reflections(1); a.context.set_sun(None, None)
        twins(a, b, 3, "toggle on, the sun off again")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_other_values_are_refused_and_the_setting_kept(built):
    from raytracedggx_amd import capi
    a, b = G.app(W, H, METAL_ARGS + SUN_ARGS), G.app(W, H, METAL_ARGS + SUN_ARGS + ["-sunreflections"])
    try:
        a.context.set_sun_reflections(1)
        for bad in (2, -1, 256):
            with pytest.raises(capi.RtggxError, match="rtggx_set_sun_reflections"):
                a.context.set_sun_reflections(bad)
        twins(a, b, 2, "refused while on")
        a.context.set_sun_reflections(0); b.context.set_sun_reflections(0)
        with pytest.raises(capi.RtggxError, match="rtggx_set_sun_reflections"):
            a.context.set_sun_reflections(3)
        twins(a, b, 2, "refused while off", denoised=False)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_strips_equal_the_full_frame(built):
    assert G.strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=tuple(SUN_ARGS) + ("-sunreflections", "-recursion", "2") + tuple(METAL_ARGS)) > 0


def test_accumulated_sums_and_a_score_record_on_the_new_words(built):
    import score_ref
    from raytracedggx_amd import capi
    a, b = G.app(W, H, METAL_ARGS + SUN_ARGS + ["-sunreflections"]), G.app(W, H, METAL_ARGS + SUN_ARGS)
    try:
        c = a.context
        c.set_accumulation(True)
        acc = AR.Accumulator(H, W)
        ref = None
        for f in range(4):
            G.frame(a); G.frame(b)
            c.sync()
            words = (c.readback(capi.BUF_TSS0 + c.frame_parity()), c.readback(capi.BUF_RT_REFL), c.readback(capi.BUF_RT_DIFF), c.readback(capi.BUF_VISIBILITY))
            assert (words[1] != G.images(b, ("refl",))["refl"]).any(), "frame %d: the words are the sun's alone" % f
            acc.add(words[1], words[2], words[3], MIXED)
            assert c.accumulated_frames() == acc.frames
            for got, want in ((c.readback(capi.BUF_ACC_REFL), acc.refl), (c.readback(capi.BUF_ACC_DIFF), acc.diff)):
                assert AR.same_bits(got, want).all(), "frame %d" % f
            if f == 0:
                ref = words[0]
                c.set_reference(ref); c.set_scoring(True)
            elif f == 1:
                recs = c.read_scores()
                assert len(recs) == 1
                want = score_ref.score(words[0], words[1], words[2], words[3], MIXED, ref, 0, None)
                bad = score_ref.same_record(recs[0], want)
                assert not bad, "frame %d: %s differ" % (f, bad)
                assert want["se_raw_rgb"] > 0.0
                c.set_scoring(False)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_a_deforming_mesh_moves_the_reflected_shadow(built):
    """gpu_support.wave, three frames at depth 2: each frame equals the restatement on the moved mesh and the refitted tree, and the set of
    pixels whose reflection is lit changes with the shape."""
    import assets
    p = hit_pair(320, 180, depth=2)
    try:
        p.frame(); G.check_raw(p, "before the deformation", require_rays=True)
        v0, idx, _ = O.obj_import(assets.path("bunny.obj"))
        lit = [p.o.lit.copy()]
        for f in range(1, 4):
            v = G.wave(v0, f)
            p.ctx.refit_as(1, v)
            p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
            p.o.set_mesh(1, v, idx)
            p.give_oracle_the_device_trees(refitted=True)
            p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
            p.o.update_as(); p.o.render_visibility(); p.rays = p.o.ray_trace()
            G.check_raw(p, "deformed, frame %d" % f, require_rays=True)
            lit.append(p.o.lit.copy())
            assert p.o.count("occluded") > 0 and lit[-1].any() and (lit[-1] != lit[-2]).any()
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()


def test_still_sky_runs_go_on_across_the_call(built):
    """A still camera and a sun: the runs of the tiles nothing is drawn in keep growing across the call, and the images equal those of a
    context that leaves no tile alone."""
    a, b = G.app(320, 180, SUN_ARGS), G.app(320, 180, SUN_ARGS)
    try:
        b.context.static_sky(False)
        before = None
        for f in range(20):
            if f == 14:
                before = a.context.sky_runs()[0].copy()
                a.context.set_sun_reflections(1); b.context.set_sun_reflections(1)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
        runs, threshold = a.context.sky_runs()
        assert (before >= threshold).any() and (runs[before >= threshold] > before[before >= threshold]).all()
    finally:
        a.OnDestroy(); b.OnDestroy()
