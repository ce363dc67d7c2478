"""One shadow ray per surface point for all local lights, on the GPU (rtggx_set_light_sampling; lighting.hip lightPickGenKernel,
lightPickAddKernel, lightHitPickGenKernel, the any-hit traversal with the rays' own intervals, sunHitAddKernel, sunHitResolveKernel): frames
bit for bit against the restatement (tests/light_pick_ref.cpp) at depth 1, at depth 2 with two samples and the lights at the hits, and
behind the sun's passes; a sample map, the other sampler and a larger sample set; one casting light against mode 0; twins; refusals; strips;
a deforming mesh; the streams; the resident launch shape; all-metal materials.  Scene and lights are those of
tests/golden/light_pick_classes.json, whose class conditions tests/test_light_pick_host.py establishes on the CPU; the tests that compare
four frames with the restatement assert them again on their own.  Every test here calls the new entry point: none passes without it."""
import json
import os

import numpy as np
import pytest

import adaptive_ref as AD
import gpu_support as G
import light_pick_ref as LP
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light_pick_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]      # 148 x 84: ragged right and bottom edges (no multiple of 8 or 16), 10 x 6 tiles
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]
FRAMES = GOLDEN["frames"]
SUN_L, SUN_E, SUN_ANGLE = [-0.6, 0.5, -0.3], [3.0, 3.0, 3.0], 5.0
SUN_ARGS = ["-sun"] + [str(x) for x in SUN_L + SUN_E]
METAL_ARGS = ["-metallic", str(MIXED[0]), str(MIXED[1])]
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
RAW = G.GBUFFER + G.RAW + G.RAYS


def light_args(lights, spot_degrees=GOLDEN["spot_degrees"]):
    """The command line of `lights`: -light for a light without a cone, -spot (with the golden file's half-angles) for one with."""
    out = []
    for l in lights:
        head = [l["position"][k] for k in range(3)] + [l["intensity"][k] for k in range(3)] + [l["range"]]
        if "cos_outer" in l:
            out += ["-spot"] + [repr(float(x)) for x in head + [l.get("radius", 0.0)] + list(l["axis"]) + list(spot_degrees)]
        else:
            out += ["-light"] + [repr(float(x)) for x in head + ([l["radius"]] if "radius" in l else [])]
    return out


def pick_pair(width, height, lights=LIGHTS, metallic=MIXED, depth=1, samples=1, sample_set=256, vndf=False, sun=False, reflections=False, mode=1):
    """gpu_support.Pair with this feature's oracle, both sides with the lights, the toggle of the lights at the hits and the mode."""
    p = G.Pair(width, height, metallic=metallic, oracle=lambda w, h: LP.Oracle(w, h, depth=depth, samples=samples, sample_set=sample_set))
    p.ctx.set_sample_set(sample_set)
    if samples != 1:
        p.ctx.set_samples_per_pixel(samples)
    if depth != 1:
        p.ctx.set_max_recursion_depth(depth)
    if vndf:
        p.ctx.set_sampler(True); p.o.set_sampler(True)
    if sun:
        p.ctx.set_sun(SUN_L, SUN_E); p.o.set_sun(SUN_L, SUN_E)
        p.ctx.set_sun_reflections(1); p.o.set_sun_reflections(True)
        p.ctx.set_sun_angle(SUN_ANGLE); p.o.set_sun_angle(SUN_ANGLE)
    p.ctx.set_lights(lights); p.o.set_lights(lights)
    p.ctx.set_light_reflections(int(reflections)); p.o.set_light_reflections(int(reflections))
    p.ctx.set_light_sampling(mode); p.o.set_light_sampling(mode)
    return p


SETTINGS = [dict(), dict(depth=2, samples=2, reflections=True), dict(sun=True, reflections=True)]
IDS = ["depth 1", "depth 2, N = 2, the lights at the hits", "behind the sun's passes and its disk, the lights at the hits"]


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_frames_equal_the_restatement(built, setting):
    """148 x 84 bunny, metallic (0.25, 0.75), the golden lights.  Four frames: G-buffer, RayTracingOut0/1 and the ray count bit for bit /
    equal, the first two also with the denoised images under the existing bars; the class conditions on the four -- of the primary pass, and
    with the lights at the hits of the hit passes."""
    p = pick_pair(W, H, **setting)
    frames = []
    try:
        for f in range(FRAMES):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            if f < 2:
                p.check_frame("frame %d" % f)
            assert p.o.light_rays > 0 and (p.o.pick_info[..., 1] != LP.NONE).any()
            if setting.get("reflections"):
                assert p.o.light_hit_rays > 0 and p.o.pick_count("lit") > 0
            frames.append(LP.record(p.o))
        got = LP.figures(frames, len(LIGHTS), bool(setting.get("reflections")))
        print("%s: %s" % (setting, got))
        LP.check_conditions(got, str(setting))
    finally:
        p.close()


@pytest.mark.parametrize("setting", [dict(samples=4, mapped=True), dict(vndf=True), dict(sample_set=1024)], ids=["N = 4 mapped 1 2 4", "VNDF", "M = 1024"])
def test_sample_maps_the_other_sampler_and_a_larger_sample_set(built, setting):
    setting = dict(setting)
    mapped = setting.pop("mapped", False)
    p = pick_pair(W, H, depth=2, reflections=True, **setting)
    try:
        blocks = None
        if mapped:
            by, bx = AD.blocks_of(W, H)
            y, x = np.mgrid[0:by, 0:bx]
            blocks = np.array([1, 2, 4], np.uint8)[(x + 2 * y) % 3]
            p.ctx.set_sample_map(blocks)
        for f in range(2):
            label = "frame %d" % f
            if mapped:
                p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
                p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
                p.o.update_as(); p.o.render_visibility()
                p.rays = LP.mapped_frame(p.o, blocks)
            else:
                p.frame()
            G.check_raw(p, label, require_rays=True)
            assert p.o.pick_count("lit", 0) > 0 and p.o.pick_count("lit", 1) > 0 and p.o.pick_count("occluded") > 0 and p.o.pick_count("two_candidates") > 0
    finally:
        p.close()


@pytest.mark.parametrize("radius", [0.0, 0.5], ids=["radius 0", "radius 0.5"])
def test_one_casting_light_is_mode_0_bit_for_bit(built, radius):
    """GPU against GPU: with one light that casts rays (and one without an intensity in front of it, which keeps the index) every pick is
    that light and f is 1 -- both images equal mode 0's, at the primary surface and at the hits, and no more rays are traced."""
    lights = [dict(LIGHTS[0], intensity=[0.0, 0.0, 0.0]), dict(LIGHTS[2], radius=radius)]
    extra = METAL_ARGS + ["-recursion", "2"]
    a, b = G.app(W, H, extra), G.app(W, H, extra)
    try:
        for x in (a, b):
            x.context.set_lights(lights); x.context.set_light_reflections(1)
        a.context.set_light_sampling(1)
        for f in range(3):
            G.frame(a); G.frame(b)
            ia, ib = G.images(a, IMAGES), G.images(b, IMAGES)
            G.assert_same({k: ia[k] for k in G.GBUFFER + G.RAW}, {k: ib[k] for k in G.GBUFFER + G.RAW}, "frame %d" % f)
            assert 0 < ia["rays"][0] <= ib["rays"][0]
    finally:
        a.OnDestroy(); b.OnDestroy()


def twins(a, b, frames, label, denoised=True):
    for f in range(frames):
        G.frame(a); G.frame(b)
        names = IMAGES if denoised else RAW
        G.assert_same(G.images(a, names), G.images(b, names), "%s, frame %d" % (label, f))
        assert a.context.placement() == b.context.placement(), "%s, frame %d: placement" % (label, f)


def test_mode_0_and_mode_1_cleared_are_a_context_that_never_calls(built):
    extra = METAL_ARGS + light_args(LIGHTS) + ["-lightreflections", "-recursion", "2"]
    a, b, c = G.app(W, H, extra), G.app(W, H, extra), G.app(W, H, extra)
    try:
        a.context.set_light_sampling(0)
        b.context.set_light_sampling(1); b.set_light_sampling(0)
        for f in range(3):
            G.frame(a); G.frame(b); G.frame(c)
            ic = G.images(c, IMAGES)
            G.assert_same(G.images(a, IMAGES), ic, "mode 0 set, frame %d" % f)
            G.assert_same(G.images(b, IMAGES), ic, "mode 1 set and cleared, frame %d" % f)
            assert a.context.placement() == c.context.placement() == b.context.placement()
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


def test_mode_1_without_lights_is_a_default_context(built):
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        a.context.set_light_sampling(1)
        twins(a, b, 3, "mode 1, no lights")
        a.context.set_lights(LIGHTS); a.context.set_lights(None)
        twins(a, b, 2, "mode 1, lights set and cleared")
        dark = [dict(l, intensity=[0.0, 0.0, 0.0]) for l in LIGHTS]
        a.context.set_lights(dark); a.context.set_light_reflections(1)
        twins(a, b, 2, "mode 1, lights that cast no ray")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_other_modes_are_refused_and_the_setting_kept(built):
    from raytracedggx_amd import capi
    extra = METAL_ARGS + light_args(LIGHTS)
    a, b = G.app(W, H, extra), G.app(W, H, extra + ["-lightpick"])
    try:
        a.context.set_light_sampling(1)
        for bad in (2, -1):
            with pytest.raises(capi.RtggxError, match="rtggx_set_light_sampling"):
                a.context.set_light_sampling(bad)
            with pytest.raises(capi.RtggxError, match="rtggx_app_set_light_sampling"):
                a.set_light_sampling(bad)
        twins(a, b, 2, "refused while in mode 1")
        c = G.app(W, H, extra)
        try:
            G.frame(c); G.frame(c)
            assert (G.images(a, G.RAW)["refl"] != G.images(c, G.RAW)["refl"]).any() and G.images(a, G.RAYS)["rays"][0] < G.images(c, G.RAYS)["rays"][0]
        finally:
            c.OnDestroy()
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_strips_equal_the_full_frame(built):
    extra = tuple(light_args(LIGHTS)) + ("-lightpick", "-lightreflections", "-recursion", "2") + tuple(METAL_ARGS)
    assert G.strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=extra) > 0


def test_a_deforming_mesh_moves_the_picks(built):
    """gpu_support.wave, three frames at depth 2: each frame equals the restatement on the moved mesh and the refitted tree."""
    import assets
    p = pick_pair(320, 180, depth=2, reflections=True)
    try:
        p.frame(); G.check_raw(p, "before the deformation", require_rays=True)
        v0, idx, _ = O.obj_import(assets.path("bunny.obj"))
        for f in range(1, 4):
            v = G.wave(v0, f)
            p.ctx.refit_as(1, v)
            p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
            p.o.set_mesh(1, v, idx)
            p.give_oracle_the_device_trees(refitted=True)
            p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
            p.o.update_as(); p.o.render_visibility(); p.rays = p.o.ray_trace()
            G.check_raw(p, "deformed, frame %d" % f, require_rays=True)
            assert p.o.pick_count("occluded") > 0 and p.o.pick_count("lit") > 0 and (p.o.pick_info[..., 2] == 5).any()
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()


def test_async_compute_off_and_a_caller_owned_stream_change_nothing(built):
    import torch
    extra = METAL_ARGS + light_args(LIGHTS) + ["-lightpick", "-lightreflections", "-recursion", "2"]
    a, b, c = G.app(320, 180, extra), G.app(320, 180, extra + ["-sync"]), G.app(320, 180, extra)
    stream = torch.cuda.Stream()
    try:
        c.context.set_stream(stream.cuda_stream)
        for f in range(6):
            for x in (a, b, c):
                x.OnUpdate(); x.OnRender()
        torch.cuda.synchronize()
        ia = G.images(a, IMAGES)
        G.assert_same(ia, G.images(b, IMAGES), "async compute off")
        G.assert_same(ia, G.images(c, IMAGES), "caller-owned stream")
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


RESIDENT = (768, 432)      # the size of test_gpu_light_hits: above RT_WIDE_RAYS = 200 000 rays, every traversal takes the resident kernel variant


def test_the_resident_launch_shape_equals_the_restatement(built):
    p = pick_pair(*RESIDENT, reflections=True)
    try:
        for f in range(2):
            p.frame()
        G.check_raw(p, "%d x %d" % RESIDENT, require_rays=True)
        assert p.rays >= 200000 and p.o.light_hit_rays >= 10000 and p.o.light_rays >= 40000, (p.rays, p.o.light_hit_rays, p.o.light_rays)
        assert p.o.pick_count("below_horizon") > 0 and p.o.pick_count("occluded") > 0
        key, where = p.ctx.placement()
        assert not key["small"] and where["shade"] == "main", (key, where)
    finally:
        p.close()


def test_all_metal_materials_leave_the_second_image_a_carry_over(built):
    """Default materials: no diffuse term and no diffuse path -- RayTracingOut1 equals the restatement's and a twin's without lights."""
    p, b = pick_pair(W, H, metallic=None, depth=2, reflections=True), G.app(W, H, ["-recursion", "2"])
    try:
        for f in range(3):
            p.frame(); G.frame(b)
            G.check_raw(p, "frame %d" % f, require_rays=True)
            ib = G.images(b, ("diff", "refl"))
            np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), ib["diff"], err_msg="frame %d: RayTracingOut1" % f)
            assert (p.ctx.readback(p.capi.BUF_RT_REFL) != ib["refl"]).any()
            assert not p.o.pick_terms[..., 3:].any() and p.o.pick_terms[..., :3].any() and p.o.pick_count("lit") > 0
    finally:
        p.close(); b.OnDestroy()
