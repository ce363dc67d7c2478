"""A list's pick weighted by what the pixel remembers, on the GPU (rtggx_set_light_list_visibility, rtggx_read_light_list_visibility;
lighting.hip lightListVisGenKernel, lightListVisAddKernel): frames bit for bit against the restatement (tests/light_list_vis_ref.cpp, which
walks ALL lights and culls nothing) under a camera that stands and then moves -- G-buffer, both traced images, the ray count, the per-block
kept counts and after every frame both record images and the sequence number --; the cull switched off; the lights at the hits at depth 2
with two samples; behind the sun's passes, with mixed and all-metal materials; list sizes around the 64-light chunk and the full 1024,
where the chosen index 1023 travels through the add; resets; where it does not act; refusals; the streams, a deforming mesh and the
resident launch shape.  Scene and list are those of tests/golden/light_list_vis_classes.json, whose class conditions
tests/test_light_list_vis_host.py establishes on the CPU over 24 frames; the frames here are twelve at the most, and the parity test asserts
again, on its own frames, the conditions twelve frames can hold.  Every test here calls the new entry point: none passes without it."""
import json
import os

import numpy as np
import pytest

import gpu_support as G
import light_list_ref as LL
import light_list_vis_ref as LV
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light_list_vis_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]      # 148 x 84: ragged right and bottom edges (no multiple of 8 or 16), 19 x 11 blocks
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]      # 73: the lattice 0 .. 63, the bright lamps behind the model 64 .. 72
LAMPS = LIGHTS[64:]
SUN_L, SUN_E, SUN_ANGLE = [-0.6, 0.5, -0.3], [3.0, 3.0, 3.0], 5.0
METAL_ARGS = ["-metallic", str(MIXED[0]), str(MIXED[1])]
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
RAW = G.GBUFFER + G.RAW + G.RAYS
SPACE = ord(" ")      # the sample's pause key: the model stops turning, or turns again


def vis_pair(width, height, lights=LIGHTS, metallic=MIXED, depth=1, samples=1, sun=False, reflections=False, vis=1):
    """gpu_support.Pair with this feature's oracle, both sides with the list, the toggle of the lights at the hits and the setting."""
    p = G.Pair(width, height, metallic=metallic, oracle=lambda w, h: LV.Oracle(w, h, depth=depth, samples=samples))
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
    p.ctx.set_light_list_visibility(vis); p.o.set_light_list_visibility(vis)
    return p


def raw_frame(p):
    """Pair.frame without the denoiser's passes on the oracle."""
    p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
    p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
    p.o.update_as(); p.o.render_visibility(); p.rays = p.o.ray_trace()


def words(records):
    return records.view(np.uint32).reshape(records.shape + (4,))


def check(p, label):
    """G-buffer, RayTracingOut0/1, the ray count, the per-block kept counts, both record images and the sequence number."""
    G.check_raw(p, label, require_rays=True)
    np.testing.assert_array_equal(p.ctx.read_light_list_counts(), p.o.list_kept, err_msg="%s: kept lights per block" % label)
    for image in (0, 1):
        got, seq = p.ctx.read_light_list_visibility(image)
        assert seq == p.o.seq, "%s: sequence %d, restatement %d" % (label, seq, p.o.seq)
        np.testing.assert_array_equal(words(got), words(p.o.images[image]), err_msg="%s: record image %d" % (label, image))


def drag(a, f):
    """The sample's orbit: the left button held over a few pixels."""
    a.OnLButtonDown(70.0, 40.0); a.OnMouseMove(70.0 + 2.0 * (f + 1), 40.0 + 1.0 * (f + 1)); a.OnLButtonUp(0.0, 0.0)


TWELVE = ("valid", "sequence", "stamp_or_instance", "normal", "inserted", "evicted", "hidden_from_64", "no_ray_carried", "lit", "occluded", "differs")      # what twelve frames can hold


def test_twelve_frames_of_a_camera_that_stands_and_then_moves_equal_the_restatement(built):
    """Test 1.  Seven frames with camera and model standing, five under an orbiting camera with the model turning.  Every frame: G-buffer,
    RayTracingOut0/1, the ray count and the kept counts bit for bit / equal, both record images and s.  An entry is freed at 63 after eight
    lit outcomes and reaches 0 after twelve occlusions at the earliest, and a tap leaves the frame only under the golden camera's jump:
    those three conditions are the host test's; the others are asserted on these frames."""
    p = vis_pair(W, H)
    frames = []
    try:
        p.app.OnKeyUp(SPACE)
        for f in range(12):
            if f == 7:
                p.app.OnKeyUp(SPACE)
            if f >= 7:
                drag(p.app, f - 7)
            raw_frame(p)
            check(p, "frame %d" % f)
            assert p.o.acted and p.o.seq == f + 1 and p.o.light_rays > 0
            frames.append(LV.counts(p.o))
        t = LV.total(frames)
        print("twelve frames: %s" % t)
        for k in TWELVE:
            assert t[k] > 0, (k, t)
        assert frames[0]["valid"] == 0 and all(fr["valid"] > 0 for fr in frames[1:])
        held = p.ctx.read_light_list_visibility(0)[0]["entry"]
        assert ((held != LV.FREE) & ((held & 1023) >= 64)).any() and ((held != LV.FREE).sum(-1) == 4).any()      # full records, lamps of the second chunk
    finally:
        p.close()


def test_the_cull_is_invisible_in_the_records_too(built):
    """Test 2.  GPU against GPU: with rtggx_debug_light_list_cull(ctx, 0) images, ray counts and both record images are the same over six
    frames of a moving camera, while the kept counts differ."""
    a, b = G.app(W, H, METAL_ARGS), G.app(W, H, METAL_ARGS)
    try:
        for x in (a, b):
            x.context.set_light_list(LIGHTS); x.set_light_list_visibility(1)
        b.context.debug_light_list_cull(0)
        for f in range(6):
            for x in (a, b):
                drag(x, f); G.frame(x)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
            for image in (0, 1):
                ra, rb = a.context.read_light_list_visibility(image), b.context.read_light_list_visibility(image)
                assert ra[1] == rb[1] == f + 1
                np.testing.assert_array_equal(words(ra[0]), words(rb[0]), err_msg="frame %d: record image %d" % (f, image))
            on, off = a.context.read_light_list_counts(), b.context.read_light_list_counts()
            assert (on <= off).all() and (on < off).any() and off.max() == LL.casting(LIGHTS)
        assert (a.context.read_light_list_visibility(0)[0]["entry"] != LV.FREE).sum() > 500
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_the_lights_at_the_hits_keep_the_lists_rule(built):
    """Test 3.  Depth 2, N = 2, rtggx_set_light_reflections(ctx, 1): four frames equal the restatement, whose hit passes are
    tests/light_list_ref.cpp's, unchanged; the records belong to the primary pass alone."""
    p = vis_pair(W, H, depth=2, samples=2, reflections=True)
    try:
        for f in range(4):
            if f >= 2:
                drag(p.app, f)
            raw_frame(p)
            check(p, "frame %d" % f)
            assert p.o.light_hit_rays > 0 and p.o.list_count("lit") > 0 and p.o.list_count("occluded") > 0 and p.o.seq == f + 1
        assert LV.counts(p.o)["valid"] > 0
    finally:
        p.close()


@pytest.mark.parametrize("metallic", [MIXED, None], ids=["mixed materials", "all-metal materials"])
def test_behind_the_suns_passes(built, metallic):
    """Test 4.  The sun with its disk and its reflections, the lights at the hits, depth 2: four frames equal the restatement.  With the
    default all-metal materials there is no diffuse term: RayTracingOut1 is that of a twin without a list."""
    p = vis_pair(W, H, metallic=metallic, depth=2, sun=True, reflections=True)
    b = None
    try:
        if metallic is None:
            b = G.app(W, H, ["-recursion", "2"])
            b.context.set_sun(SUN_L, SUN_E); b.context.set_sun_reflections(1); b.context.set_sun_angle(SUN_ANGLE)
        for f in range(4):
            raw_frame(p)
            check(p, "frame %d" % f)
            if b is not None:
                G.frame(b)
                ib = G.images(b, ("diff", "refl"))
                np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), ib["diff"], err_msg="frame %d: RayTracingOut1" % f)
                assert (p.ctx.readback(p.capi.BUF_RT_REFL) != ib["refl"]).any()
                assert not p.o.list_terms[..., 3:].any() and p.o.list_terms[..., :3].any()
        c = LV.counts(p.o)
        assert c["valid"] > 0 and c["occluded"] > 0 and c["lit"] > 0, c
    finally:
        p.close()
        if b is not None:
            b.OnDestroy()


def sized_list(n):
    """n lights whose LAST ones are the bright lamps behind the model (so that the highest indices are chosen, found hidden and recorded),
    in front of them the lattice repeated with shifted positions."""
    lamps = LAMPS[len(LAMPS) - min(n, len(LAMPS)):]
    out = []
    for k in range(n - len(lamps)):
        l, r = dict(LIGHTS[k % 64]), k // 64
        l["position"] = [round(l["position"][0] + 0.37 * r - 1.8, 3), round(l["position"][1] + 0.05 * r, 3), round(l["position"][2] + 0.29 * r - 1.5, 3)] if r else list(l["position"])
        out.append(l)
    return out + lamps


@pytest.mark.parametrize("n", [1, 9, 64, 65, 1024])
def test_list_sizes(built, n):
    """Test 5.  One light; the nine lamps; a full chunk, one beyond it, all 1024: four standing frames each against the restatement.  The
    last light of every list is the brightest hidden lamp: its index -- 1023 in the full list -- is chosen, travels through the add in ten
    bits and stands in the records.  A list of one gives the list's own images bit for bit (f = 1), compared with a twin without the setting."""
    lights = sized_list(n)
    assert len(lights) == n
    p = vis_pair(W, H, lights=lights)
    b = G.app(W, H, METAL_ARGS) if n == 1 else None
    try:
        p.app.OnKeyUp(SPACE)
        if b is not None:
            b.OnKeyUp(SPACE); b.context.set_light_list(lights)
        for f in range(4):
            raw_frame(p)
            check(p, "%d lights, frame %d" % (n, f))
            if b is not None:
                G.frame(b)
                G.assert_same(G.images(p.app, RAW), G.images(b, RAW), "one light, frame %d" % f)
                assert (p.o.list_wf[p.o.list_info[..., 1] != LL.NONE, 1] == 1.0).all()
        entries = p.ctx.read_light_list_visibility(0)[0]["entry"]
        last = (entries != LV.FREE) & ((entries & 1023) == n - 1)
        assert last.sum() > 20 and ((entries[last] >> 10) < LV.INSERT).any(), (n, int(last.sum()))      # inserted, and found hidden again
        assert (p.o.list_info[..., 1] == n - 1).any()
        if n >= 64:
            assert p.o.list_kept.max() > 8
    finally:
        p.close()
        if b is not None:
            b.OnDestroy()


def test_a_new_list_and_a_toggle_are_frames_without_history(built):
    """Test 6.  rtggx_set_light_list with the same list behind the third frame, the setting off and on behind the fifth: the frame after
    each equals the restatement's frame in which no pixel has valid history, and its records are those of a context that acts for the first
    time in that frame -- a twin that ran beside it with the setting off: the same entries and normal words, the stamps s = 1."""
    p = vis_pair(W, H)
    twins = {3: G.app(W, H, METAL_ARGS), 5: G.app(W, H, METAL_ARGS)}
    try:
        p.app.OnKeyUp(SPACE)
        for t in twins.values():
            t.OnKeyUp(SPACE); t.context.set_light_list(LIGHTS)
        for f in range(7):
            if f == 3:
                p.ctx.set_light_list(LIGHTS); p.o.set_light_list(LIGHTS)
            if f == 5:
                for x in (p.ctx, p.o):
                    x.set_light_list_visibility(0); x.set_light_list_visibility(1)
            if f in twins:
                twins[f].context.set_light_list_visibility(1)
            raw_frame(p)
            for t in twins.values():
                G.frame(t)
            check(p, "frame %d" % f)
            cls = p.o.vis_info[..., 0]
            if f in (0, 3, 5):
                assert (cls == LV.VALID).sum() == 0 and (cls == LV.SEQUENCE).sum() > 0, f
            else:
                assert (cls == LV.VALID).sum() > 0, f
            if f in twins:
                mine, s = p.ctx.read_light_list_visibility((f + 1) & 1)
                fresh, s1 = twins[f].context.read_light_list_visibility(1)
                assert s == f + 1 and s1 == 1
                written = (mine["stamp"] >> 8) == f + 1
                assert written.sum() > 2000 and np.array_equal(written, (fresh["stamp"] >> 8) == 1)
                for k in ("entry", "normal"):
                    np.testing.assert_array_equal(mine[k][written], fresh[k][written], err_msg="frame %d: %s against a first acting frame" % (f, k))
                np.testing.assert_array_equal(mine["stamp"][written] & 0xFF, fresh["stamp"][written] & 0xFF)
                assert ((mine["entry"][written] != LV.FREE).sum(-1) <= 1).all() and (mine["entry"][written] != LV.FREE).any()      # one insert at the most
    finally:
        p.close()
        for t in twins.values():
            t.OnDestroy()


def test_where_it_does_not_act_the_context_is_one_that_never_called(built):
    """Test 7.  Enabled on a context with rtggx_set_lights and no list (modes 0 and 1), with a list of dark lights, and without lights at
    all: images, ray counts and placement are those of the same run without the call, and nothing is allocated -- the records cannot be read."""
    from raytracedggx_amd import capi
    eight = LAMPS[:8]
    dark = [dict(l, intensity=[0.0, 0.0, 0.0]) for l in LIGHTS]
    cases = (("rtggx_set_lights, mode 0", lambda x: x.context.set_lights(eight)), ("rtggx_set_lights, mode 1", lambda x: (x.context.set_lights(eight), x.context.set_light_sampling(1))),
             ("a dark list", lambda x: x.context.set_light_list(dark)), ("no lights", lambda x: None))
    for label, prepare in cases:
        a, b = G.app(W, H, METAL_ARGS), G.app(W, H, METAL_ARGS)
        try:
            prepare(a); prepare(b)
            with pytest.raises(capi.RtggxError, match="rtggx_read_light_list_visibility"):
                a.context.read_light_list_visibility(0)
            a.context.set_light_list_visibility(1)
            for f in range(3):
                G.frame(a); G.frame(b)
                G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "%s, frame %d" % (label, f))
                assert a.context.placement() == b.context.placement(), "%s, frame %d: placement" % (label, f)
                with pytest.raises(capi.RtggxError, match="rtggx_read_light_list_visibility: no records yet"):
                    a.context.read_light_list_visibility(0)
        finally:
            a.OnDestroy(); b.OnDestroy()


def test_other_values_and_strips_are_refused_and_everything_stays(built):
    """Test 8."""
    import ctypes as C
    from raytracedggx_amd import capi
    a, b, c = G.app(W, H, METAL_ARGS), G.app(W, H, METAL_ARGS), G.app(W, H, METAL_ARGS)
    try:
        for x in (a, b, c):
            x.context.set_light_list(LIGHTS)
        a.context.set_light_list_visibility(1); b.set_light_list_visibility(1)
        for bad in (2, -1):
            with pytest.raises(capi.RtggxError, match="rtggx_set_light_list_visibility"):
                a.context.set_light_list_visibility(bad)
            with pytest.raises(capi.RtggxError, match="rtggx_app_set_light_list_visibility"):
                a.set_light_list_visibility(bad)
        with pytest.raises(capi.RtggxError, match="rtggx_set_strip.*rtggx_set_light_list_visibility.*whole frames only"):
            a.context.set_strip(0, H // 2)      # a strip on an enabled context
        c.context.set_strip(16, H)
        with pytest.raises(capi.RtggxError, match="rtggx_set_light_list_visibility: on a strip.*whole frames only"):
            c.context.set_light_list_visibility(1)      # enabling on a context with a strip
        c.context.set_strip(0, H)
        for f in range(3):
            G.frame(a); G.frame(b); G.frame(c)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "refused while enabled, frame %d" % f)
            for image in (0, 1):
                ra, rb = a.context.read_light_list_visibility(image), b.context.read_light_list_visibility(image)
                assert ra[1] == rb[1] == f + 1 and np.array_equal(words(ra[0]), words(rb[0]))
            with pytest.raises(capi.RtggxError, match="rtggx_read_light_list_visibility"):
                c.context.read_light_list_visibility(0)      # the refused context stayed a plain list
        with pytest.raises(capi.RtggxError, match="rtggx_read_light_list_visibility: image 2"):
            a.context.read_light_list_visibility(2)
        out, seq = np.zeros((H, W), capi.LIGHT_LIST_VIS_RECORD), C.c_uint32(99)
        for nbytes in (out.nbytes - 16, out.nbytes + 16, 0):
            assert a.context.L.rtggx_read_light_list_visibility(a.context.h, 0, out.ctypes.data_as(C.c_void_p), nbytes, C.byref(seq)) != 0
        assert seq.value == 99 and not words(out).any()
        assert a.context.read_light_list_visibility(1)[1] == 3
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


def list_file(tmp_path, lights=LIGHTS):
    lines = ["light " + " ".join(repr(float(x)) for x in list(l["position"]) + list(l["intensity"]) + [l["range"]] + ([l["radius"]] if "radius" in l else [])) for l in lights]
    path = tmp_path / "lights.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_async_compute_off_and_a_caller_owned_stream_change_nothing(built, tmp_path):
    """Test 9, the streams: six frames with -lightlistvisibility; images and both record images identical with -sync and on a stream of the caller's."""
    import torch
    extra = METAL_ARGS + ["-lightlist", list_file(tmp_path), "-lightlistvisibility", "-lightreflections", "-recursion", "2"]
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
            ra = a.context.read_light_list_visibility(image)
            assert ra[1] == 6 and (ra[0]["entry"] != LV.FREE).any()
            for x, label in ((b, "async compute off"), (c, "caller-owned stream")):
                rx = x.context.read_light_list_visibility(image)
                assert rx[1] == 6 and np.array_equal(words(ra[0]), words(rx[0])), "%s: record image %d" % (label, image)
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


def test_a_deforming_mesh_carries_its_records_along(built):
    """Test 9, a deforming mesh: gpu_support.wave, three frames at 320 x 180, each equal to the restatement on the moved mesh and the
    refitted tree."""
    import assets
    p = vis_pair(320, 180)
    try:
        raw_frame(p); check(p, "before the deformation")
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
            c = LV.counts(p.o)
            assert c["valid"] > 0 and c["occluded"] > 0 and c["lit"] > 0, c
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()


RESIDENT = (768, 432)      # the size of test_gpu_light_list: above RT_WIDE_RAYS = 200 000 rays, every traversal takes the resident kernel variant


def test_the_resident_launch_shape_equals_the_restatement(built):
    """Three frames at the size of tests/test_gpu_light_list.py's test of that shape, the launch shape pinned to the wide one as
    tests/test_gpu_light_vis.py pins it."""
    p = vis_pair(*RESIDENT, reflections=True)
    try:
        p.ctx.placement(force_small=0)
        for f in range(3):
            raw_frame(p)
        check(p, "%d x %d" % RESIDENT)
        c = LV.counts(p.o)
        assert p.rays >= 200000 and p.o.light_rays >= 40000 and c["valid"] > 40000 and c["differs"] > 0, (p.rays, p.o.light_rays, c)
        key, where = p.ctx.placement()
        assert not key["small"] and where["shade"] == "main", (key, where)
    finally:
        p.close()
