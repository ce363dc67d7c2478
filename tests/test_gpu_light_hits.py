"""The local lights at the surfaces the paths hit, on the GPU (rtggx_set_light_reflections; lighting.hip lightHitGenKernel, the any-hit
traversal with the rays' own intervals, sunHitAddKernel, sunHitResolveKernel): frames bit for bit against the restatement
(tests/light_hit_ref.cpp) at depth 1 to 3, with several samples, a sample map, the other sampler and a larger sample set; behind the sun's
hit pass in the shared sums; the lights without radii; both bin sizes; preset returns; twins; refusals; accumulation; strips; a deforming
mesh; still sky; the resident launch shape.  Scene and lights are those of tests/golden/light_hit_classes.json, whose class conditions
tests/test_light_hit_host.py establishes on the CPU; the tests that compare four frames with the restatement assert them again on their own."""
import json
import os

import numpy as np
import pytest

import accum_ref as AR
import adaptive_ref as AD
import gpu_support as G
import light_hit_ref as LH
import lights_ref as LR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light_hit_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]      # 148 x 84: ragged right and bottom edges (no multiple of 8 or 16), 10 x 6 tiles
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]
FRAMES = GOLDEN["frames"]
RADII = [l.get("radius", 0.0) for l in LIGHTS]
DARK = [dict(l, intensity=[0.0, 0.0, 0.0]) for l in LIGHTS]
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


def hit_pair(width, height, lights=LIGHTS, metallic=MIXED, depth=1, samples=1, sample_set=256, vndf=False, sun=False):
    """gpu_support.restated_pair with this feature's oracle, both sides with the lights and the toggle on."""
    p = G.Pair(width, height, metallic=metallic, oracle=lambda w, h: LH.Oracle(w, h, depth=depth, samples=samples, sample_set=sample_set))
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
    p.ctx.set_light_reflections(1); p.o.set_light_reflections(1)
    return p


def record(o):
    return o.light_counts.copy(), o.light_cls0.copy(), o.light_hit_rays


SETTINGS = [dict(), dict(depth=2, samples=2), dict(depth=3), dict(sun=True)]
IDS = ["depth 1", "depth 2, N = 2", "depth 3", "behind the sun's hit pass and its disk"]


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_frames_equal_the_restatement(built, setting):
    """148 x 84 bunny, metallic (0.25, 0.75) -- 128-slot bins in two compaction rounds, both lobes, ragged edges --, the three lights.  Four
    frames: G-buffer, RayTracingOut0/1 and the ray count bit for bit / equal, the first two also with the denoised images under the existing
    bars; the class conditions on the four.  With the sun: the shared S, the order sun-then-lights, the single resolve."""
    p = hit_pair(W, H, **setting)
    frames = []
    try:
        for f in range(FRAMES):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            if f < 2:
                p.check_frame("frame %d" % f)
            assert p.o.light_hit_rays > 0 and p.o.light_rays > 0
            if setting.get("sun"):
                assert p.o.count("lit") > 0 and (p.o.lit & ~p.o.light_lit).any() and ((p.o.light_lit & 1) != 0).any()
            frames.append(record(p.o))
        got = LH.figures(frames, len(LIGHTS))
        print("%s: %s" % (setting, got))
        LH.check_conditions(got, RADII, str(setting), setting.get("depth", 1))
    finally:
        p.close()


@pytest.mark.parametrize("setting", [dict(samples=4, mapped=True), dict(vndf=True), dict(sample_set=1024)], ids=["N = 4 mapped 1 2 4", "VNDF", "M = 1024"])
def test_sample_maps_the_other_sampler_and_a_larger_sample_set(built, setting):
    setting = dict(setting)
    mapped = setting.pop("mapped", False)
    p = hit_pair(W, H, depth=2, **setting)
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
                p.rays = LH.mapped_frame(p.o, blocks)
            else:
                p.frame()
            G.check_raw(p, label, require_rays=True)
            assert p.o.light_count("lit", 0) > 0 and p.o.light_count("lit", 1) > 0 and p.o.light_count("occluded") > 0 and p.o.light_lit.any()
    finally:
        p.close()


def test_without_radii_no_hit_is_below_the_horizon(built):
    """The three lights with rho = 0 -- the variants of the generating kernel without the hash: three frames at depth 2, the class empty."""
    p = hit_pair(W, H, lights=[dict(l, radius=0.0) for l in LIGHTS], depth=2)
    try:
        for f in range(3):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            assert p.o.light_count("below_horizon") == 0 and p.o.light_count("occluded") > 0 and p.o.light_count("outside_cone") > 0 and p.o.light_count("lit", 1) > 0
    finally:
        p.close()


def test_all_metal_64_slot_bins_and_the_carry_over(built):
    """Default materials: bins of 64 slots, no diffuse path -- RayTracingOut1 equals the restatement's and a twin's without the toggle."""
    p, b = hit_pair(W, H, metallic=None, depth=2), G.app(W, H, ["-recursion", "2"] + light_args(LIGHTS))
    try:
        for f in range(3):
            p.frame(); G.frame(b)
            G.check_raw(p, "frame %d" % f, require_rays=True)
            ib = G.images(b, ("diff", "refl", "rays"))
            np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), ib["diff"], err_msg="frame %d: RayTracingOut1" % f)
            assert (p.ctx.readback(p.capi.BUF_RT_REFL) != ib["refl"]).any() and p.ctx.ray_count() == ib["rays"][0] + p.o.light_hit_rays
            assert p.o.light_count("lit", 0) > 0 and p.o.light_count("lit", 1) > 0 and p.o.light_count("lit_diffuse") == 0 and not (p.o.light_lit & 2).any()
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
            assert p.o.count("preset") > 0 and p.o.light_hit_rays > 0
    finally:
        p.close()


def twins(a, b, frames, label, denoised=True):
    for f in range(frames):
        G.frame(a); G.frame(b)
        names = IMAGES if denoised else RAW
        G.assert_same(G.images(a, names), G.images(b, names), "%s, frame %d" % (label, f))
        assert a.context.placement() == b.context.placement(), "%s, frame %d: placement" % (label, f)


def test_the_toggle_without_lights_is_a_default_context(built):
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        a.context.set_light_reflections(1)
        twins(a, b, 3, "toggle on, no lights")
        a.context.set_lights(LIGHTS); a.context.set_lights(None)
        twins(a, b, 2, "toggle on, lights set and cleared")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_the_toggle_turned_off_again_is_the_lights_alone(built):
    extra = METAL_ARGS + light_args(LIGHTS)
    a, b = G.app(320, 180, extra), G.app(320, 180, extra)
    try:
        a.context.set_light_reflections(1); a.context.set_light_reflections(0)
        twins(a, b, 2, "on and off before the first frame")
        a.set_light_reflections(1)
        for f in range(3):
            G.frame(a); G.frame(b)
            ia, ib = G.images(a, IMAGES), G.images(b, IMAGES)
            assert ia["rays"][0] > ib["rays"][0] and (ia["refl"] != ib["refl"]).any() and (ia["diff"] != ib["diff"]).any()
            G.assert_same({k: ia[k] for k in G.GBUFFER}, {k: ib[k] for k in G.GBUFFER}, "toggle on, frame %d" % f)
        a.context.set_light_reflections(0)
        twins(a, b, 6, "toggle off again", denoised=False)      # (the temporal history forgets the earlier frames geometrically)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_the_toggle_with_lights_that_cast_no_ray_changes_no_buffer(built):
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        a.context.set_lights(DARK); b.context.set_lights(DARK)
        a.context.set_light_reflections(1)
        twins(a, b, 3, "all intensities 0")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_the_suns_toggle_alone_never_hears_of_the_new_function(built):
    """A context with the sun's toggle and this one, but no lights, against one that never calls the new function -- and both with lights but
    only the sun's toggle."""
    extra = METAL_ARGS + SUN_ARGS + ["-sunreflections", "-recursion", "2"]
    a, b = G.app(W, H, extra), G.app(W, H, extra)
    try:
        a.context.set_light_reflections(1)
        twins(a, b, 3, "the sun's toggle, this one without lights")
        a.context.set_light_reflections(0); a.context.set_lights(LIGHTS); b.context.set_lights(LIGHTS)
        twins(a, b, 2, "the sun's toggle and lights", denoised=False)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_other_values_are_refused_and_the_setting_kept(built):
    from raytracedggx_amd import capi
    extra = METAL_ARGS + light_args(LIGHTS)
    a, b = G.app(W, H, extra), G.app(W, H, extra + ["-lightreflections"])
    try:
        a.context.set_light_reflections(1)
        for bad in (2, -1, 256):
            with pytest.raises(capi.RtggxError, match="rtggx_set_light_reflections"):
                a.context.set_light_reflections(bad)
            with pytest.raises(capi.RtggxError, match="rtggx_app_set_light_reflections"):
                a.set_light_reflections(bad)
        twins(a, b, 2, "refused while on")
        a.context.set_light_reflections(0); b.set_light_reflections(0)
        with pytest.raises(capi.RtggxError, match="rtggx_set_light_reflections"):
            a.context.set_light_reflections(3)
        twins(a, b, 2, "refused while off", denoised=False)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_lights_taken_away_leave_the_frames_of_a_default_context(built):
    """Two lit frames with the toggle, then no lights: RayTracingOut0/1 and the ray count are a default context's again (S was left zero) --
    and the lights given back light the hits again."""
    a, b = G.app(W, H, METAL_ARGS), G.app(W, H, METAL_ARGS)
    try:
        a.context.set_lights(LIGHTS); a.context.set_light_reflections(1)
        for f in range(2):
            G.frame(a); G.frame(b)
            assert (G.images(a, G.RAW)["refl"] != G.images(b, G.RAW)["refl"]).any()
        a.context.set_lights(None)
        for f in range(2):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, RAW), G.images(b, RAW), "frame %d without" % f)
        a.context.set_lights(LIGHTS); b.context.set_lights(LIGHTS)
        G.frame(a); G.frame(b)
        assert G.images(a, G.RAYS)["rays"][0] > G.images(b, G.RAYS)["rays"][0]
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_accumulated_sums_equal_the_restatements(built):
    """4 accumulated frames: the sums bit for bit against accum_ref over the restatement's frames."""
    from raytracedggx_amd import capi
    p = hit_pair(W, H)
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
    extra = tuple(light_args(LIGHTS)) + ("-lightreflections", "-recursion", "2") + tuple(METAL_ARGS)
    assert G.strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=extra) > 0


def test_a_deforming_mesh_moves_the_reflected_shadows(built):
    """gpu_support.wave, three frames at depth 2: each frame equals the restatement on the moved mesh and the refitted tree."""
    import assets
    p = hit_pair(320, 180, depth=2)
    try:
        p.frame(); G.check_raw(p, "before the deformation", require_rays=True)
        v0, idx, _ = O.obj_import(assets.path("bunny.obj"))
        lit = [p.o.light_lit.copy()]
        for f in range(1, 4):
            v = G.wave(v0, f)
            p.ctx.refit_as(1, v)
            p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
            p.o.set_mesh(1, v, idx)
            p.give_oracle_the_device_trees(refitted=True)
            p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
            p.o.update_as(); p.o.render_visibility(); p.rays = p.o.ray_trace()
            G.check_raw(p, "deformed, frame %d" % f, require_rays=True)
            lit.append(p.o.light_lit.copy())
            assert p.o.light_count("occluded") > 0 and lit[-1].any() and (lit[-1] != lit[-2]).any()
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()


def test_async_compute_off_and_a_caller_owned_stream_change_nothing(built):
    import torch
    extra = METAL_ARGS + light_args(LIGHTS) + ["-lightreflections", "-recursion", "2"]
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
    """A still camera and lights: the runs of the tiles nothing is drawn in keep growing across the call, and the images equal those of a
    context that leaves no tile alone."""
    extra = METAL_ARGS + light_args(LIGHTS)
    a, b = G.app(320, 180, extra), G.app(320, 180, extra)
    try:
        b.context.static_sky(False)
        before = None
        for f in range(20):
            if f == 14:
                before = a.context.sky_runs()[0].copy()
                a.context.set_light_reflections(1); b.context.set_light_reflections(1)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
        runs, threshold = a.context.sky_runs()
        assert (before >= threshold).any() and (runs[before >= threshold] > before[before >= threshold]).all()
    finally:
        a.OnDestroy(); b.OnDestroy()


RESIDENT = (768, 432)      # ~0.9 rays per pixel with these materials and lights: above RT_WIDE_RAYS = 200 000 rays, where a frame's launches
#                            are no longer small and every traversal -- the hits' too -- takes the resident kernel variant (RT_TINY_RAYS = 40 000)


def test_the_resident_launch_shape_equals_the_restatement(built):
    """The second of two frames at the smallest 16:9 size whose ray count is safely above RT_WIDE_RAYS: the rays' own intervals in the
    resident kernel variant and 128-slot bins, on the main stream and its spill part.  Raw words and ray counts against the restatement."""
    p = hit_pair(*RESIDENT)
    try:
        for f in range(2):
            p.frame()
        G.check_raw(p, "%d x %d" % RESIDENT, require_rays=True)
        assert p.rays >= 200000 and p.o.light_hit_rays >= 20000, (p.rays, p.o.light_hit_rays)
        assert p.o.light_count("below_horizon") > 0 and p.o.light_count("occluded") > 0
        key, where = p.ctx.placement()
        assert not key["small"] and where["shade"] == "main", (key, where)
    finally:
        p.close()


def query_rays(n=300, seed=31):
    """A short list through the scene's box, every ray with an interval of its own: (tmin, tmax) in (0 .. 0.5, 1 .. 30)."""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = rng.uniform((-8.0, -2.0, -8.0), (8.0, 8.0, 8.0), (n, 3))
    d = rng.normal(size=(n, 3)); r[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 6] = rng.uniform(0.0, 0.5, n); r[:, 7] = rng.uniform(1.0, 30.0, n)
    return r


@pytest.mark.parametrize("at", [0, 2], ids=["queries before the first frame", "queries between frames"])
def test_ray_queries_and_the_lit_frames_leave_each_other_alone(built, at):
    """Every queue of a frame states its own shape to the traversal -- the frame's 128-slot bins, the sun's and the lights' 64-slot bins with
    and without the rays' intervals, the two hit passes' queues -- and so does the list of rtggx_trace_rays / rtggx_trace_occlusion, which
    borrows a set's bins and brings intervals of its own.  Metallic below 1, the three lights, the sun, both toggles: the frames of a context
    that makes both queries equal those of a twin that makes none, in every buffer and the ray count, and the queries' results equal those
    of a fresh context -- default materials (64-slot bins), no sun, no lights -- brought to the same frame."""
    extra = METAL_ARGS + light_args(LIGHTS) + SUN_ARGS + ["-sunreflections", "-lightreflections"]
    a, b, fresh = G.app(W, H, extra), G.app(W, H, extra), G.app(W, H)
    rays = query_rays()
    try:
        for f in range(at + 2):
            for x in (a, b) + ((fresh,) if f <= at else ()):
                x.OnUpdate()
            if f == at:      # (the constants of frame `at` are in place, its kernels are not launched yet)
                got, occ = a.context.trace_rays(rays), a.context.trace_occlusion(rays)
                want, occ_fresh = fresh.context.trace_rays(rays), fresh.context.trace_occlusion(rays)
                G.assert_same(got, want, "trace_rays at frame %d" % f)
                np.testing.assert_array_equal(occ, occ_fresh, err_msg="trace_occlusion at frame %d" % f)
                np.testing.assert_array_equal(occ, got["valid"])
                assert occ.any() and not occ.all()
            for x in (a, b) + ((fresh,) if f < at else ()):
                x.OnRender()
            ia = G.images(a, IMAGES)
            G.assert_same(ia, G.images(b, IMAGES), "frame %d" % f)
            assert ia["rays"][0] > 0
    finally:
        a.OnDestroy(); b.OnDestroy(); fresh.OnDestroy()
