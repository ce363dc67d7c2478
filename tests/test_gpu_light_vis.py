"""The pick weighted by what the pixel remembers, on the GPU (rtggx_set_light_pick_visibility, rtggx_read_light_visibility; lighting.hip
lightPickVisGenKernel, lightPickVisAddKernel): frames bit for bit against the restatement (tests/light_vis_ref.cpp) under a camera that moves
and then stands -- G-buffer, both traced images, the ray count and after every frame both record images and the sequence number -- at depth 1
and at depth 2 with two samples, the lights at the hits and the sun; a long standing run that reaches the floor and 0; one casting light
against mode 0; twins; resets; refusals; a deforming mesh; the streams; the resident launch shape; all-metal materials.  Scene and lights are
those of tests/golden/light_vis_classes.json.  Every test here calls the new entry point: none passes without it."""
import json
import os

import numpy as np
import pytest

import gpu_support as G
import light_pick_ref as LP
import light_vis_ref as LV
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light_vis_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]      # 148 x 84: ragged right and bottom edges (no multiple of 8 or 16), 10 x 6 tiles
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]
SUN_L, SUN_E, SUN_ANGLE = [-0.6, 0.5, -0.3], [3.0, 3.0, 3.0], 5.0
METAL_ARGS = ["-metallic", str(MIXED[0]), str(MIXED[1])]
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
SPACE = ord(" ")      # the sample's pause key: the model stops turning


def light_args(lights, spot_degrees=GOLDEN["spot_degrees"]):
    """The command line of `lights` (tests/test_gpu_light_pick.py)."""
    out = []
    for l in lights:
        head = [l["position"][k] for k in range(3)] + [l["intensity"][k] for k in range(3)] + [l["range"]]
        if "cos_outer" in l:
            out += ["-spot"] + [repr(float(x)) for x in head + [l.get("radius", 0.0)] + list(l["axis"]) + list(spot_degrees)]
        else:
            out += ["-light"] + [repr(float(x)) for x in head + ([l["radius"]] if "radius" in l else [])]
    return out


def vis_pair(width, height, lights=LIGHTS, metallic=MIXED, depth=1, samples=1, sun=False, reflections=False, mode=1, vis=1):
    """gpu_support.Pair with this feature's oracle, both sides with the lights, the mode and the setting."""
    p = G.Pair(width, height, metallic=metallic, oracle=lambda w, h: LV.Oracle(w, h, depth=depth, samples=samples))
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
    p.ctx.set_light_reflections(int(reflections)); p.o.set_light_reflections(int(reflections))
    p.ctx.set_light_sampling(mode); p.o.set_light_sampling(mode)
    p.ctx.set_light_pick_visibility(vis); p.o.set_light_pick_visibility(vis)
    return p


def raw_frame(p):
    """Pair.frame without the denoiser's passes on the oracle."""
    p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
    p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
    p.o.update_as(); p.o.render_visibility(); p.rays = p.o.ray_trace()


def check_records(p, label):
    """Both record images and the sequence number against the restatement's."""
    for image in (0, 1):
        got, seq = p.ctx.read_light_visibility(image)
        assert seq == p.o.seq, "%s: sequence %d, restatement %d" % (label, seq, p.o.seq)
        np.testing.assert_array_equal(got.view(np.uint32).reshape(p.o.H, p.o.W, 4), p.o.images[image].view(np.uint32).reshape(p.o.H, p.o.W, 4),
                                      err_msg="%s: record image %d" % (label, image))


def drag(p, f):
    """The sample's orbit: the left button held over a few pixels."""
    p.app.OnLButtonDown(70.0, 40.0); p.app.OnMouseMove(70.0 + 2.0 * (f + 1), 40.0 + 1.0 * (f + 1)); p.app.OnLButtonUp(0.0, 0.0)


EIGHT = ("valid", "sequence", "off_frame", "stamp", "instance", "normal", "v255", "lit", "occluded", "no_ray", "differs")      # what eight frames can hold


@pytest.mark.parametrize("setting", [dict(), dict(depth=2, samples=2, reflections=True, sun=True)], ids=["depth 1", "depth 2, N = 2, the lights at the hits, the sun"])
def test_eight_frames_of_a_camera_that_moves_and_then_stands_equal_the_restatement(built, setting):
    """Four frames under an orbiting camera and a turning model, four with both standing.  Every frame: G-buffer, RayTracingOut0/1 and the ray
    count bit for bit / equal, both record images and s.  At depth 2 the hits run mode 1's rule: the oracle's walker is light_pick_ref's.
    The class conditions that eight frames can hold are asserted on these frames: a byte is below the floor after ten occlusions in a row at
    the earliest and at 0 after seventeen (test_a_standing_run_reaches_the_floor_and_zero)."""
    p = vis_pair(W, H, **setting)
    frames = []
    try:
        for f in range(8):
            if f < 4:
                drag(p, f)
            elif f == 4:
                p.app.OnKeyUp(SPACE)
            raw_frame(p)
            G.check_raw(p, "frame %d" % f, require_rays=True)
            check_records(p, "frame %d" % f)
            assert p.o.acted and p.o.seq == f + 1 and p.o.light_rays > 0
            if setting.get("reflections"):
                assert p.o.light_hit_rays > 0 and p.o.pick_count("lit") > 0
            frames.append(LV.counts(p.o))
        t = LV.total(frames)
        print("%s: %s" % (setting, t))
        for k in EIGHT:
            assert t[k] > 0, (k, t)
        assert frames[0]["valid"] == 0 and all(fr["valid"] > 0 for fr in frames[1:])
    finally:
        p.close()


def test_a_standing_run_reaches_the_floor_and_zero(built):
    """Twenty frames with camera and model standing, each bit for bit: candidates below the floor and at 0 appear, and fewer rays are wasted
    at the end than at the start."""
    p = vis_pair(W, H)
    frames = []
    try:
        p.app.OnKeyUp(SPACE)
        for f in range(20):
            raw_frame(p)
            G.check_raw(p, "frame %d" % f, require_rays=True)
            check_records(p, "frame %d" % f)
            frames.append(LV.counts(p.o))
        t = LV.total(frames)
        print("standing: %s" % t)
        assert t["floor"] > 0 and t["v0"] > 0 and t["v255"] > 0 and t["differs"] > 0, t
        assert frames[-1]["occluded"] < frames[0]["occluded"], (frames[0], frames[-1])
    finally:
        p.close()


@pytest.mark.parametrize("radius", [0.0, 0.5], ids=["radius 0", "radius 0.5"])
def test_one_casting_light_is_mode_0_bit_for_bit(built, radius):
    """GPU against GPU: with one light that casts rays (behind one without an intensity, which keeps the index) every pick is that light and f
    is 1 whatever the byte holds -- both images and the ray count equal mode 0's over four frames, while the records fill."""
    lights = [dict(LIGHTS[1], intensity=[0.0, 0.0, 0.0]), dict(LIGHTS[0], radius=radius)]
    a, b = G.app(W, H, METAL_ARGS), G.app(W, H, METAL_ARGS)
    try:
        for x in (a, b):
            x.context.set_lights(lights)
        a.context.set_light_sampling(1); a.context.set_light_pick_visibility(1)
        for f in range(4):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, G.GBUFFER + G.RAW + G.RAYS), G.images(b, G.GBUFFER + G.RAW + G.RAYS), "frame %d" % f)
        rec, seq = a.context.read_light_visibility(0)
        assert seq == 4 and (rec["v"][..., 1] < 128).any() and (rec["stamp"] >> 8 == 4).any()
    finally:
        a.OnDestroy(); b.OnDestroy()


def twins(a, b, frames, label):
    from raytracedggx_amd import capi
    for f in range(frames):
        G.frame(a); G.frame(b)
        G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "%s, frame %d" % (label, f))
        assert a.context.placement() == b.context.placement(), "%s, frame %d: placement" % (label, f)
        with pytest.raises(capi.RtggxError, match="rtggx_read_light_visibility"):
            a.context.read_light_visibility(0)


def test_where_it_does_not_act_the_context_is_one_that_never_called(built):
    """Enabled without lights; enabled in mode 0; enabled and disabled again before the first frame: images, ray counts, placement -- and
    nothing is allocated, so the records cannot be read."""
    lit = METAL_ARGS + light_args(LIGHTS)
    for label, extra, prepare in (("enabled without lights", METAL_ARGS + [], lambda x: (x.context.set_light_sampling(1), x.context.set_light_pick_visibility(1))),
                                  ("enabled in mode 0", lit, lambda x: x.context.set_light_pick_visibility(1)),
                                  ("enabled then disabled", lit + ["-lightpick"], lambda x: (x.set_light_pick_visibility(1), x.context.set_light_pick_visibility(0)))):
        a, b = G.app(W, H, extra), G.app(W, H, extra)
        try:
            prepare(a)
            twins(a, b, 3, label)
        finally:
            a.OnDestroy(); b.OnDestroy()


def test_set_lights_in_mid_sequence_is_a_frame_without_history(built):
    """The same list set again behind the third frame: the fourth equals the restatement's frame in which no pixel has valid history (and
    differs from the frame of an undisturbed twin); the fifth has history again.  So does a change of the mode and back."""
    p, q = vis_pair(W, H), vis_pair(W, H)
    try:
        for x in (p, q):
            x.app.OnKeyUp(SPACE)
        for f in range(6):
            if f == 3:
                p.ctx.set_lights(LIGHTS); p.o.set_lights(LIGHTS)
            if f == 5:
                p.ctx.set_light_sampling(1); p.o.set_light_sampling(1)
            raw_frame(p); raw_frame(q)
            G.check_raw(p, "frame %d" % f, require_rays=True); check_records(p, "frame %d" % f)
            check_records(q, "twin, frame %d" % f)
            cls = p.o.vis_info[..., 0]
            if f in (0, 3, 5):
                assert (cls == LV.VALID).sum() == 0 and (cls == LV.SEQUENCE).sum() > 0, f
            else:
                assert (cls == LV.VALID).sum() > 0, f
            if f == 3:
                assert (p.ctx.read_light_visibility(0)[0]["v"] != q.ctx.read_light_visibility(0)[0]["v"]).any()
    finally:
        p.close(); q.close()


def test_other_values_and_strips_are_refused_and_everything_stays(built):
    from raytracedggx_amd import capi
    extra = METAL_ARGS + light_args(LIGHTS) + ["-lightpick"]
    a, b, c = G.app(W, H, extra), G.app(W, H, extra + ["-lightvisibility"]), G.app(W, H, extra)
    try:
        a.context.set_light_pick_visibility(1)
        for bad in (2, -1):
            with pytest.raises(capi.RtggxError, match="rtggx_set_light_pick_visibility"):
                a.context.set_light_pick_visibility(bad)
            with pytest.raises(capi.RtggxError, match="rtggx_app_set_light_pick_visibility"):
                a.set_light_pick_visibility(bad)
        with pytest.raises(capi.RtggxError, match="rtggx_set_strip.*rtggx_set_light_pick_visibility.*whole frames only"):
            a.context.set_strip(0, H // 2)      # a strip on an enabled context
        c.context.set_strip(16, H)
        with pytest.raises(capi.RtggxError, match="rtggx_set_light_pick_visibility: on a strip.*whole frames only"):
            c.context.set_light_pick_visibility(1)      # enabling on a context with a strip
        c.context.set_strip(0, H)
        for f in range(3):
            G.frame(a); G.frame(b); G.frame(c)
            ia = G.images(a, IMAGES)
            G.assert_same(ia, G.images(b, IMAGES), "refused while enabled, frame %d" % f)
            for image in (0, 1):
                ra, rb = a.context.read_light_visibility(image), b.context.read_light_visibility(image)
                assert ra[1] == rb[1] == f + 1 and np.array_equal(ra[0], rb[0])
            with pytest.raises(capi.RtggxError, match="rtggx_read_light_visibility"):
                c.context.read_light_visibility(0)      # the refused context stayed in plain mode 1
        with pytest.raises(capi.RtggxError, match="rtggx_read_light_visibility"):
            a.context.read_light_visibility(2)
        assert (G.images(a, G.RAW)["refl"] != G.images(c, G.RAW)["refl"]).any()
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


def test_a_deforming_mesh_carries_its_records_along(built):
    """gpu_support.wave, three frames: each equals the restatement on the moved mesh and the refitted tree."""
    import assets
    p = vis_pair(320, 180)
    try:
        raw_frame(p); G.check_raw(p, "before the deformation", require_rays=True); check_records(p, "before the deformation")
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
            check_records(p, "deformed, frame %d" % f)
            c = LV.counts(p.o)
            assert c["valid"] > 0 and c["occluded"] > 0 and c["lit"] > 0, c
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()


def test_async_compute_off_and_a_caller_owned_stream_change_nothing(built):
    import torch
    extra = METAL_ARGS + light_args(LIGHTS) + ["-lightpick", "-lightvisibility", "-lightreflections", "-recursion", "2"]
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
        for image in (0, 1):
            ra = a.context.read_light_visibility(image)
            assert ra[1] == 6
            for x, label in ((b, "async compute off"), (c, "caller-owned stream")):
                rx = x.context.read_light_visibility(image)
                assert rx[1] == 6 and np.array_equal(ra[0], rx[0]), "%s: record image %d" % (label, image)
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


RESIDENT = (768, 432)      # the size of test_gpu_light_hits: above RT_WIDE_RAYS = 200 000 rays, every traversal takes the resident kernel variant


def test_the_resident_launch_shape_equals_the_restatement(built):
    """Three frames at the size of tests/test_gpu_light_hits.py, the launch shape pinned to the wide one (the frame's first launch has about
    RT_WIDE_RAYS rays here, so left to the counters the shape depends on which launch they were sampled behind)."""
    p = vis_pair(*RESIDENT, reflections=True)
    try:
        p.ctx.placement(force_small=0)
        for f in range(3):
            raw_frame(p)
        G.check_raw(p, "%d x %d" % RESIDENT, require_rays=True)
        check_records(p, "%d x %d" % RESIDENT)
        c = LV.counts(p.o)
        assert p.rays >= 200000 and p.o.light_rays >= 40000 and c["valid"] > 40000 and c["differs"] > 0, (p.rays, p.o.light_rays, c)
        key, where = p.ctx.placement()
        assert not key["small"] and where["shade"] == "main", (key, where)
    finally:
        p.close()


def test_all_metal_materials_leave_the_second_image_a_carry_over(built):
    """Default materials: no diffuse term -- RayTracingOut1 equals the restatement's and a twin's without lights, while the records fill."""
    p, b = vis_pair(W, H, metallic=None), G.app(W, H, [])
    try:
        for f in range(3):
            raw_frame(p); G.frame(b)
            G.check_raw(p, "frame %d" % f, require_rays=True)
            check_records(p, "frame %d" % f)
            ib = G.images(b, ("diff", "refl"))
            np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), ib["diff"], err_msg="frame %d: RayTracingOut1" % f)
            assert (p.ctx.readback(p.capi.BUF_RT_REFL) != ib["refl"]).any()
            assert not p.o.pick_terms[..., 3:].any() and p.o.pick_terms[..., :3].any()
    finally:
        p.close(); b.OnDestroy()
