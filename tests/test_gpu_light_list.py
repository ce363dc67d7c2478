"""A light list beyond eight, on the GPU (rtggx_set_light_list; lighting.hip lightListGenKernel, lightListHitGenKernel, and mode 1's
lightPickAddKernel, any-hit traversal, sunHitAddKernel and sunHitResolveKernel behind them): frames and per-block kept counts bit for bit
against the restatement (tests/light_list_ref.cpp), which walks ALL lights and culls nothing, at depth 1, at depth 2 with two samples and
the lights at the hits, and behind the sun's passes; a list of eight against the same lights through rtggx_set_lights in mode 1; the cull
switched off; list sizes around the 64-light chunk and the full 1024; twins; refusals; strips; a deforming mesh; the streams; the resident
launch shape; all-metal materials.  Scene and list are those of tests/golden/light_list_classes.json, whose class conditions
tests/test_light_list_host.py establishes on the CPU; the test that compares four frames with the restatement asserts them again on its
own.  Every test here calls the new entry point: none passes without it.
The hits' cull has no counts of its own: one that keeps too little shows in the images of the depth-2 frames, one that keeps everything
only in time."""
import json
import os

import numpy as np
import pytest

import gpu_support as G
import light_list_ref as LL
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light_list_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]      # 148 x 84: ragged right and bottom edges (no multiple of 8 or 16), 19 x 11 blocks
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]
FRAMES = GOLDEN["frames"]
CASTING = LL.casting(LIGHTS)
SUN_L, SUN_E, SUN_ANGLE = [-0.6, 0.5, -0.3], [3.0, 3.0, 3.0], 5.0
METAL_ARGS = ["-metallic", str(MIXED[0]), str(MIXED[1])]
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
RAW = G.GBUFFER + G.RAW + G.RAYS


def list_file(tmp_path, lights=LIGHTS):
    """A -lightlist file of `lights` (the golden file's half-angles for the cones)."""
    lines = []
    for l in lights:
        head = list(l["position"]) + list(l["intensity"]) + [l["range"]]
        if "cos_outer" in l:
            lines.append("spot " + " ".join(repr(float(x)) for x in head + [l.get("radius", 0.0)] + list(l["axis"]) + list(GOLDEN["spot_degrees"])))
        else:
            lines.append("light " + " ".join(repr(float(x)) for x in head + ([l["radius"]] if "radius" in l else [])))
    path = tmp_path / "lights.txt"
    path.write_text("# the golden list\n" + "\n".join(lines) + "\n")
    return str(path)


def list_pair(width, height, lights=LIGHTS, metallic=MIXED, depth=1, samples=1, sun=False, reflections=False):
    """gpu_support.Pair with this feature's oracle, both sides with the list and the toggle of the lights at the hits."""
    p = G.Pair(width, height, metallic=metallic, oracle=lambda w, h: LL.Oracle(w, h, depth=depth, samples=samples))
    if samples != 1:
        p.ctx.set_samples_per_pixel(samples)
    if depth != 1:
        p.ctx.set_max_recursion_depth(depth)
    if sun:
        p.ctx.set_sun(SUN_L, SUN_E); p.o.set_sun(SUN_L, SUN_E)
        p.ctx.set_sun_reflections(1); p.o.set_sun_reflections(True)
        p.ctx.set_sun_angle(SUN_ANGLE); p.o.set_sun_angle(SUN_ANGLE)
    p.ctx.set_light_list(lights); p.o.set_light_list(lights)
    p.ctx.set_light_reflections(int(reflections)); p.o.set_light_reflections(int(reflections))
    return p


def check(p, label):
    """check_raw, and the per-block kept counts against the cull's restatement."""
    G.check_raw(p, label, require_rays=True)
    np.testing.assert_array_equal(p.ctx.read_light_list_counts(), p.o.list_kept, err_msg="%s: kept lights per block" % label)


SETTINGS = [dict(), dict(depth=2, samples=2, reflections=True), dict(sun=True, reflections=True)]
IDS = ["depth 1", "depth 2, N = 2, the lights at the hits", "behind the sun's passes and its disk, the lights at the hits"]


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_frames_equal_the_restatement(built, setting):
    """148 x 84 bunny, metallic (0.25, 0.75), the golden list of 96.  Four frames: G-buffer, RayTracingOut0/1, the ray count and the
    per-block counts bit for bit / equal, the first two also with the denoised images under the existing bars; the class conditions on the
    four -- of the blocks, of the primary pass, and with the lights at the hits of the level-0 hits."""
    p = list_pair(W, H, **setting)
    frames, both = [], []
    try:
        for f in range(FRAMES):
            p.frame()
            check(p, "frame %d" % f)
            if f < 2:
                p.check_frame("frame %d" % f)
            assert p.o.light_rays > 0 and (p.o.list_info[..., 1] != LL.NONE).any()
            if setting.get("reflections"):
                assert p.o.light_hit_rays > 0 and p.o.list_count("lit") > 0
            frames.append(LL.record(p.o))
            both.append(LL.block_kept_chunks(p.o).all(0))
        got = LL.figures(frames, CASTING, both, bool(setting.get("reflections")))
        print("%s: %s" % (setting, got))
        # one light's range covers everything: the blocks that keep nothing are those of the first 65 lights (test_list_sizes)
        assert got["blocks"]["none_kept"] == 0
        LL.check_conditions(dict(got, blocks=dict(got["blocks"], none_kept=GOLDEN["prefix65"]["none_kept"])), str(setting))
    finally:
        p.close()


def test_a_short_list_is_the_same_lights_in_mode_1(built):
    """GPU against GPU: the first 8 golden lights as a list equal the same 8 through rtggx_set_lights in mode 1 -- all images and the ray
    count, at depth 2 with the lights at the hits."""
    lights = LIGHTS[:8]
    extra = METAL_ARGS + ["-recursion", "2"]
    a, b, c = G.app(W, H, extra), G.app(W, H, extra), G.app(W, H, extra)
    try:
        a.context.set_light_list(lights); a.context.set_light_reflections(1)
        b.context.set_lights(lights); b.context.set_light_reflections(1); b.context.set_light_sampling(1)
        for f in range(3):
            G.frame(a); G.frame(b); G.frame(c)
            ia = G.images(a, IMAGES)
            G.assert_same(ia, G.images(b, IMAGES), "frame %d" % f)
            ic = G.images(c, RAW)
            assert ia["rays"][0] > ic["rays"][0] and (ia["refl"] != ic["refl"]).any() and (ia["diff"] != ic["diff"]).any()
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


def test_the_cull_is_invisible_and_it_culls(built):
    """GPU against GPU: with rtggx_debug_light_list_cull(ctx, 0) the images and ray counts are the same, at depth 2 with the lights at the
    hits, and every block with a covered pixel reads the number of casting lights; with the cull most blocks read far fewer."""
    from raytracedggx_amd import capi
    extra = METAL_ARGS + ["-recursion", "2"]
    a, b = G.app(W, H, extra), G.app(W, H, extra)
    try:
        for x in (a, b):
            x.context.set_light_list(LIGHTS); x.context.set_light_reflections(1)
        b.context.debug_light_list_cull(0)
        for bad in (2, -1):
            with pytest.raises(capi.RtggxError, match="rtggx_debug_light_list_cull"):
                b.context.debug_light_list_cull(bad)
        for f in range(3):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
            covered = LL.block_covered(G.images(a, ("vis",))["vis"] != 0)
            on, off = a.context.read_light_list_counts(), b.context.read_light_list_counts()
            assert covered.sum() > 60
            np.testing.assert_array_equal(off, np.where(covered, CASTING, 0))
            assert (on <= off).all() and (on[covered] > 0).all() and (4 * on[covered] < CASTING).sum() >= 8 and not on[~covered].any()
        b.context.debug_light_list_cull(1)
        G.frame(a); G.frame(b)
        np.testing.assert_array_equal(a.context.read_light_list_counts(), b.context.read_light_list_counts())
    finally:
        a.OnDestroy(); b.OnDestroy()


def big_list(n):
    """The golden list repeated with shifted positions, n lights."""
    out = []
    for k in range(n):
        l, r = dict(LIGHTS[k % len(LIGHTS)]), k // len(LIGHTS)
        l["position"] = [round(l["position"][0] + 0.37 * r - 1.8, 3), round(l["position"][1] + 0.05 * r, 3), round(l["position"][2] + 0.29 * r - 1.5, 3)] if r else list(l["position"])
        out.append(l)
    return out


@pytest.mark.parametrize("n", [1, 9, 63, 64, 65, 1024])
def test_list_sizes(built, n):
    """One light; one beyond eight; one below, at and beyond a chunk of 64; all 1024: two frames each at depth 1 against the restatement,
    images, ray count and per-block counts.  1025 are refused.  The lists up to 65 do not hold the light that covers everything: blocks
    with a covered pixel keep nothing."""
    lights = big_list(n)
    p = list_pair(W, H, lights=lights)
    none_kept = 0
    try:
        with pytest.raises(p.capi.RtggxError, match="rtggx_set_light_list: 1025 lights: at most 1024"):
            p.ctx.set_light_list(big_list(1025))
        for f in range(2):
            p.frame()
            check(p, "%d lights, frame %d" % (n, f))
            covered = LL.block_covered(p.o.buffer(O.BUF_VISIBILITY) != 0)
            none_kept += int((covered & (p.o.list_kept == 0)).sum())
            if n >= 63:
                assert p.o.list_kept.max() > 8 and (p.o.list_info[..., 1] >= 8)[p.o.list_info[..., 1] != LL.NONE].any()
            if n == 1024:
                assert none_kept == 0 and p.o.list_kept.max() > 64 and ((p.o.list_info[..., 1] >= 512) & (p.o.list_info[..., 1] != LL.NONE)).any()
        assert n > 65 or none_kept >= LL.MIN_BLOCKS, none_kept      # (the golden file's prefix65: the still scene's figure over four frames)
    finally:
        p.close()


def twins(a, b, frames, label, names=IMAGES):
    for f in range(frames):
        G.frame(a); G.frame(b)
        G.assert_same(G.images(a, names), G.images(b, names), "%s, frame %d" % (label, f))
        assert a.context.placement() == b.context.placement(), "%s, frame %d: placement" % (label, f)


def test_a_list_set_and_cleared_and_a_dark_list_are_a_context_that_never_calls(built):
    from raytracedggx_amd import capi
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        a.context.set_light_list(LIGHTS); a.context.set_light_list(None)
        twins(a, b, 3, "a list set and cleared")
        a.set_light_list(LIGHTS); G.frame(a); G.frame(b)
        assert (G.images(a, G.RAW)["refl"] != G.images(b, G.RAW)["refl"]).any()
        a.set_light_list([])
        twins(a, b, 2, "a list rendered with and cleared", RAW)      # (the history still holds the lit frame: the frame's own words)
    finally:
        a.OnDestroy(); b.OnDestroy()
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        with pytest.raises(capi.RtggxError, match="rtggx_read_light_list_counts"):
            a.context.read_light_list_counts()
        dark = [dict(l, intensity=[0.0, 0.0, 0.0]) for l in LIGHTS]
        a.context.set_light_list(dark); a.context.set_light_reflections(1)
        with pytest.raises(capi.RtggxError, match="rtggx_read_light_list_counts"):      # (set, and no frame yet)
            a.context.read_light_list_counts()
        twins(a, b, 3, "a list of dark lights")
        assert not a.context.read_light_list_counts().any()      # a light without intensity is never kept
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_refusals_keep_what_the_context_holds(built):
    from raytracedggx_amd import capi
    extra = METAL_ARGS
    a, b = G.app(W, H, extra), G.app(W, H, extra)
    try:
        a.context.set_light_list(LIGHTS); b.context.set_light_list(LIGHTS)
        with pytest.raises(capi.RtggxError, match="rtggx_set_lights: .*rtggx_set_light_list"):
            a.context.set_lights(LIGHTS[:3])
        a.context.set_lights(None)      # (nothing to hold: accepted)
        with pytest.raises(capi.RtggxError, match="rtggx_set_light_list: 1025 lights"):
            a.context.set_light_list(LIGHTS * 10 + LIGHTS[:65])
        with pytest.raises(capi.RtggxError, match="rtggx_set_light_list: light 5: a range"):
            a.context.set_light_list([dict(l, range=(-1.0 if i == 5 else l["range"])) for i, l in enumerate(LIGHTS)])
        with pytest.raises(capi.RtggxError, match="rtggx_set_light_list: light 95: intensity"):
            a.context.set_light_list([dict(l, intensity=([1.0, float("nan"), 1.0] if i == 95 else l["intensity"])) for i, l in enumerate(LIGHTS)])
        with pytest.raises(capi.RtggxError, match="rtggx_set_light_list: light 68: the axis"):
            a.context.set_light_list([dict(l, axis=([0.0, 0.0, 0.0] if i == 68 else l.get("axis", [0.0, 0.0, 0.0]))) for i, l in enumerate(LIGHTS)])
        with pytest.raises(capi.RtggxError, match="rtggx_app_set_light_list|rtggx_set_light_list"):
            a.set_light_list([dict(l, radius=(99.0 if i == 0 else l.get("radius", 0.0))) for i, l in enumerate(LIGHTS)])
        with pytest.raises(capi.RtggxError, match="rtggx_set_ray_rate"):
            a.context.set_ray_rate(4)
        twins(a, b, 2, "refused calls while a list is held")
        assert a.context.read_light_list_counts().max() > 8
        c = G.app(W, H, extra)
        try:
            c.context.set_lights(LIGHTS[:3])
            with pytest.raises(capi.RtggxError, match="rtggx_set_light_list: .*rtggx_set_lights"):
                c.context.set_light_list(LIGHTS)
            c.context.set_light_list(None)
            c.context.set_ray_rate(1)
            G.frame(c)
            with pytest.raises(capi.RtggxError, match="rtggx_read_light_list_counts"):
                c.context.read_light_list_counts()
        finally:
            c.OnDestroy()
        a.context.set_strip(8, H - 8)
        try:
            with pytest.raises(capi.RtggxError, match="rtggx_read_light_list_counts: on a strip"):
                a.context.read_light_list_counts()
        finally:
            a.context.set_strip(0, H)
        d = capi.Context(64, 64)
        try:
            d.set_ray_rate(4)
            with pytest.raises(capi.RtggxError, match="rtggx_set_light_list: .*rtggx_set_ray_rate"):
                d.set_light_list(LIGHTS)
        finally:
            d.close()
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_strips_equal_the_full_frame(built, tmp_path):
    extra = ("-lightlist", list_file(tmp_path), "-lightreflections", "-recursion", "2") + tuple(METAL_ARGS)
    assert G.strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=extra) > 0


def test_the_list_file_is_the_list(built, tmp_path):
    """-lightlist with the golden list equals rtggx_set_light_list with it: the cones' cosines are the command line's."""
    a, b = G.app(W, H, METAL_ARGS + ["-lightlist", list_file(tmp_path)]), G.app(W, H, METAL_ARGS)
    try:
        b.context.set_light_list(LIGHTS)
        twins(a, b, 2, "-lightlist")
        np.testing.assert_array_equal(a.context.read_light_list_counts(), b.context.read_light_list_counts())
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_a_deforming_mesh_moves_the_picks(built):
    """gpu_support.wave, three frames at depth 2: each frame equals the restatement on the moved mesh and the refitted tree."""
    import assets
    p = list_pair(320, 180, depth=2, reflections=True)
    try:
        p.frame(); check(p, "before the deformation")
        v0, idx, _ = O.obj_import(assets.path("bunny.obj"))
        for f in range(1, 4):
            v = G.wave(v0, f)
            p.ctx.refit_as(1, v)
            p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
            p.o.set_mesh(1, v, idx)
            p.give_oracle_the_device_trees(refitted=True)
            p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
            p.o.update_as(); p.o.render_visibility(); p.rays = p.o.ray_trace()
            check(p, "deformed, frame %d" % f)
            assert p.o.list_count("occluded") > 0 and p.o.list_count("lit") > 0 and (p.o.list_info[..., 2] == 5).any()
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()


def test_async_compute_off_and_a_caller_owned_stream_change_nothing(built, tmp_path):
    import torch
    extra = METAL_ARGS + ["-lightlist", list_file(tmp_path), "-lightreflections", "-recursion", "2"]
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
        np.testing.assert_array_equal(a.context.read_light_list_counts(), b.context.read_light_list_counts())
        np.testing.assert_array_equal(a.context.read_light_list_counts(), c.context.read_light_list_counts())
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


RESIDENT = (768, 432)      # the size of test_gpu_light_hits: above RT_WIDE_RAYS = 200 000 rays, every traversal takes the resident kernel variant


def test_the_resident_launch_shape_equals_the_restatement(built):
    p = list_pair(*RESIDENT, reflections=True)
    try:
        for f in range(2):
            p.frame()
        check(p, "%d x %d" % RESIDENT)
        assert p.rays >= 200000 and p.o.light_hit_rays >= 10000 and p.o.light_rays >= 40000, (p.rays, p.o.light_hit_rays, p.o.light_rays)
        assert p.o.list_count("below_horizon") > 0 and p.o.list_count("occluded") > 0
        key, where = p.ctx.placement()
        assert not key["small"] and where["shade"] == "main", (key, where)
    finally:
        p.close()


def test_all_metal_materials_leave_the_second_image_a_carry_over(built):
    """Default materials: no diffuse term and no diffuse path -- RayTracingOut1 equals the restatement's and a twin's without a list."""
    p, b = list_pair(W, H, metallic=None, depth=2, reflections=True), G.app(W, H, ["-recursion", "2"])
    try:
        for f in range(3):
            p.frame(); G.frame(b)
            check(p, "frame %d" % f)
            ib = G.images(b, ("diff", "refl"))
            np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), ib["diff"], err_msg="frame %d: RayTracingOut1" % f)
            assert (p.ctx.readback(p.capi.BUF_RT_REFL) != ib["refl"]).any()
            assert not p.o.list_terms[..., 3:].any() and p.o.list_terms[..., :3].any() and p.o.list_count("lit") > 0
    finally:
        p.close(); b.OnDestroy()
