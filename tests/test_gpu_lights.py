"""Local lights on the GPU (rtggx_set_lights; lighting.hip lightGenKernel, lightAddKernel): frames bit for bit against the restatement
(tests/lights_ref.cpp) at depth 1, at depth 2 with two samples and behind the sun's passes; the three lights without their radii; all-metal
materials; twins; refusals; the command line; accumulation; strips; a deforming mesh; still sky; the resident launch shape.  Scene and lights
are those of tests/golden/lights_classes.json, whose class conditions tests/test_lights_host.py establishes on the CPU; the tests that
compare frames with the restatement assert them again on their own frames."""
import json
import os

import numpy as np
import pytest

import accum_ref as AR
import gpu_support as G
import lights_ref as LR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lights_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]      # 148 x 84: ragged right and bottom edges (no multiple of 8 or 16), 10 x 6 tiles
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]
FRAMES = GOLDEN["frames"]
SUN_L, SUN_E, SUN_ANGLE = [-0.6, 0.5, -0.3], [3.0, 3.0, 3.0], 5.0
METAL_ARGS = ["-metallic", str(MIXED[0]), str(MIXED[1])]
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS


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


def lights_pair(width, height, lights=LIGHTS, metallic=MIXED, depth=1, samples=1, sun=False):
    """gpu_support.restated_pair with this feature's oracle, both sides with the lights."""
    p = G.Pair(width, height, metallic=metallic, oracle=lambda w, h: LR.Oracle(w, h, depth=depth, samples=samples))
    p.ctx.set_sample_set(256)
    if samples != 1:
        p.ctx.set_samples_per_pixel(samples)
    if depth != 1:
        p.ctx.set_max_recursion_depth(depth)
    if sun:
        p.ctx.set_sun(SUN_L, SUN_E); p.o.set_sun(SUN_L, SUN_E)
        p.ctx.set_sun_reflections(1); p.o.set_sun_reflections(True)
        p.ctx.set_sun_angle(SUN_ANGLE); p.o.set_sun_angle(SUN_ANGLE)
    p.ctx.set_lights(lights); p.o.set_lights(lights)
    p.o.statistics_lights = True
    return p


SETTINGS = [dict(), dict(depth=2, samples=2), dict(sun=True)]
IDS = ["depth 1", "depth 2, N = 2", "behind the sun, its reflections and its disk"]


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_frames_equal_the_restatement(built, setting):
    """148 x 84 bunny, metallic (0.25, 0.75), the three lights.  Four frames: G-buffer, RayTracingOut0/1 and the ray count bit for bit /
    equal, the first two also with the denoised images under the existing bars; the class conditions on the four."""
    p = lights_pair(W, H, **setting)
    classes, aux = [], []
    try:
        for f in range(FRAMES):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            if f < 2:
                p.check_frame("frame %d" % f)
            assert p.o.light_rays > 0
            classes.append(p.o.light_classes.copy()); aux.append(p.o.light_aux.copy())
        got = LR.figures(np.stack(classes), np.stack(aux))
        print("%s: %s" % (setting, got))
        LR.check_conditions(got, str(setting))
    finally:
        p.close()


def test_without_radii_no_pixel_is_below_the_horizon(built):
    """The three lights with rho = 0 -- the variants of the generating kernel without the hash: three frames, and class 4 empty."""
    p = lights_pair(W, H, lights=[dict(l, radius=0.0) for l in LIGHTS])
    try:
        for f in range(3):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            assert not (p.o.light_classes == LR.BELOW_HORIZON).any() and (p.o.light_classes == LR.OCCLUDED).any() and (p.o.light_classes == LR.OUTSIDE_CONE).any()
    finally:
        p.close()


def test_all_metal_leaves_the_carry_over_alone(built):
    """Default materials: no diffuse path -- RayTracingOut1 equals the restatement's and a lightless twin's, RayTracingOut0 does not."""
    p, b = lights_pair(W, H, metallic=None), G.app(W, H)
    try:
        for f in range(3):
            p.frame(); G.frame(b)
            G.check_raw(p, "frame %d" % f, require_rays=True)
            ib = G.images(b, ("diff", "refl"))
            np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), ib["diff"], err_msg="frame %d: RayTracingOut1" % f)
            assert (p.ctx.readback(p.capi.BUF_RT_REFL) != ib["refl"]).any()
    finally:
        p.close(); b.OnDestroy()


def twins(a, b, frames, label):
    for f in range(frames):
        G.frame(a); G.frame(b)
        G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "%s, frame %d" % (label, f))
        assert a.context.placement() == b.context.placement(), "%s, frame %d: placement" % (label, f)


def test_lights_set_and_cleared_before_the_next_frame_are_a_default_context(built):
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        twins(a, b, 1, "before")
        a.context.set_lights(LIGHTS); a.context.set_lights(None)
        twins(a, b, 3, "lights set and cleared")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_count_0_from_the_start_is_a_default_context(built):
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        a.context.set_lights([]); a.set_lights(None)
        twins(a, b, 3, "count == 0; and b never calls it")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_lights_taken_away_leave_the_frames_of_a_default_context(built):
    """Two lit frames, then none: RayTracingOut0/1 and the ray count are a default context's again (the sums were left zero)."""
    a, b = G.app(W, H, METAL_ARGS), G.app(W, H, METAL_ARGS)
    names = G.GBUFFER + G.RAW + G.RAYS
    try:
        a.context.set_lights(LIGHTS)
        for f in range(2):
            G.frame(a); G.frame(b)
            assert (G.images(a, G.RAW)["refl"] != G.images(b, G.RAW)["refl"]).any()
        a.context.set_lights(None)
        for f in range(2):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, names), G.images(b, names), "frame %d without" % f)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_the_flags_are_the_call(built):
    a, b, dark = G.app(W, H, METAL_ARGS + light_args(LIGHTS)), G.app(W, H, METAL_ARGS), G.app(W, H, METAL_ARGS)
    try:
        b.set_lights(LIGHTS)
        twins(a, b, 2, "-light and -spot")
        G.frame(dark); G.frame(dark)
        assert (G.images(a, G.RAW)["refl"] != G.images(dark, G.RAW)["refl"]).any()
    finally:
        a.OnDestroy(); b.OnDestroy(); dark.OnDestroy()


def test_refused_lists_leave_the_lights_as_they_were(built):
    from raytracedggx_amd import capi
    p = lights_pair(W, H)
    ok = dict(position=[0.0, 5.0, 0.0], intensity=[1.0, 1.0, 1.0], range=10.0)
    nan, inf = float("nan"), float("inf")
    bad = [dict(position=[nan, 0, 0]), dict(range=0.0), dict(range=inf), dict(range=nan), dict(intensity=[1, -1.0, 1]), dict(intensity=[0, inf, 0]),
           dict(radius=-0.1), dict(radius=10.0), dict(radius=nan), dict(cos_outer=0.5, cos_inner=0.9), dict(cos_outer=0.5, cos_inner=0.9, axis=[nan, 1, 0]),
           dict(axis=[0, 1, 0], cos_outer=0.5, cos_inner=0.5), dict(axis=[0, 1, 0], cos_outer=0.5, cos_inner=1.5), dict(axis=[0, 1, 0], cos_outer=nan, cos_inner=0.5)]
    try:
        p.frame(); G.check_raw(p, "before", require_rays=True)
        for b in bad:
            for lights in ([dict(ok, **b)], [ok, ok, dict(ok, **b)]):      # a list is taken whole or not at all
                with pytest.raises(capi.RtggxError, match="rtggx_set_lights"):
                    p.ctx.set_lights(lights)
                with pytest.raises(ValueError):
                    p.o.set_lights(lights)
        with pytest.raises(capi.RtggxError, match="rtggx_set_lights"):
            p.ctx.set_lights([ok] * 9)
        with pytest.raises(ValueError):
            p.o.set_lights([ok] * 9)
        assert p.ctx.L.rtggx_set_lights(p.ctx.h, None, 2) != 0      # a null pointer with a count
        with pytest.raises(capi.RtggxError, match="rtggx_set_ray_rate"):
            p.ctx.set_ray_rate(4)
        p.frame(); G.check_raw(p, "after the refusals", require_rays=True)
        assert p.o.light_rays > 0 and p.o.light_classes.shape[0] == len(LIGHTS)
        p.ctx.set_lights([ok] * 8); p.o.set_lights([ok] * 8)      # the cap itself is allowed
        p.frame(); G.check_raw(p, "eight lights", require_rays=True)
    finally:
        p.close()
    q = G.app(W, H, ["-rayrate", "4"])
    try:
        with pytest.raises(capi.RtggxError, match="rtggx_set_lights"):
            q.context.set_lights(LIGHTS)
        q.context.set_lights(None)      # (turning them off is no request for lights)
    finally:
        q.OnDestroy()


def test_accumulated_sums_equal_the_restatements(built):
    """4 accumulated frames: the sums bit for bit against accum_ref over the restatement's frames."""
    from raytracedggx_amd import capi
    p = lights_pair(W, H)
    try:
        c = p.ctx
        c.set_accumulation(True)
        acc = AR.Accumulator(H, W)
        for f in range(4):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            acc.add(p.o.buffer(O.BUF_RT_REFL), p.o.buffer(O.BUF_RT_DIFF), p.o.buffer(O.BUF_VISIBILITY), MIXED)
            assert c.accumulated_frames() == acc.frames
            for got, want in ((c.readback(capi.BUF_ACC_REFL), acc.refl), (c.readback(capi.BUF_ACC_DIFF), acc.diff)):
                assert AR.same_bits(got, want).all(), "frame %d" % f
    finally:
        p.close()


def test_strips_equal_the_full_frame(built):
    extra = tuple(light_args(LIGHTS)) + tuple(METAL_ARGS)
    assert G.strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=extra) > 0


def test_a_deforming_mesh_moves_the_shadows(built):
    """gpu_support.wave, three frames: each frame equals the restatement on the moved mesh and the refitted tree."""
    import assets
    p = lights_pair(320, 180)
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
            assert (p.o.light_classes == LR.OCCLUDED).any() and (p.o.light_classes == LR.LIT).any()
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()


def test_async_compute_off_and_a_caller_owned_stream_change_nothing(built):
    import torch
    extra = METAL_ARGS + light_args(LIGHTS)
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


def test_still_sky_runs_go_on_across_the_call(built):
    """A still camera: the runs of the tiles nothing is drawn in keep growing across the call, and the images equal those of a context that
    leaves no tile alone."""
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        b.context.static_sky(False)
        before = None
        for f in range(20):
            if f == 14:
                before = a.context.sky_runs()[0].copy()
                a.context.set_lights(LIGHTS); b.context.set_lights(LIGHTS)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
        runs, threshold = a.context.sky_runs()
        assert (before >= threshold).any() and (runs[before >= threshold] > before[before >= threshold]).all()
    finally:
        a.OnDestroy(); b.OnDestroy()


RESIDENT = (768, 432)      # ~0.9 rays per pixel with these materials and lights: above RT_WIDE_RAYS = 200 000 rays, where a frame's launches
#                            are no longer small and every traversal -- the lights' too -- takes the resident kernel variant (RT_TINY_RAYS = 40 000)


def test_the_resident_launch_shape_equals_the_restatement(built):
    """The second of two frames at the smallest 16:9 size whose ray count is safely above RT_WIDE_RAYS: raw words and ray counts against
    the restatement, statistics off."""
    p = lights_pair(*RESIDENT)
    p.o.statistics_lights = False
    try:
        for f in range(2):
            p.frame()
        G.check_raw(p, "%d x %d" % RESIDENT, require_rays=True)
        assert p.rays >= 200000 and p.o.light_rays >= 40000, (p.rays, p.o.light_rays)
        assert (p.o.light_classes == LR.BELOW_HORIZON).any() and (p.o.light_classes == LR.OCCLUDED).any()
        key, where = p.ctx.placement()
        assert not key["small"] and where["shade"] == "main", (key, where)
    finally:
        p.close()
