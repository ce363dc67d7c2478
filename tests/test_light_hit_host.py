"""The local lights at the surfaces the paths hit, the part that needs no GPU: rtggx_set_light_reflections declared, exported and bound, and
the header's rule; -lightreflections checked at parse time; the restatement (tests/light_hit_ref.cpp) against tests/lights_ref.cpp's frames
with the toggle off, without lights and with lights that cast no ray; what the toggle may and may not change; the hash slots worked out
apart from it; and the class conditions of the scene the GPU tests use (tests/golden/light_hit_classes.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import host_support as HS
import light_hit_ref as LH
import lights_ref as LR
from oracle import oracle as O

GOLDEN = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "light_hit_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]
FRAMES = GOLDEN["frames"]
RADII = [l.get("radius", 0.0) for l in LIGHTS]
SUN = ([-0.6, 0.5, -0.3], [3.0, 3.0, 3.0])
SMALL = (100, 56)      # the frames that are only compared with each other


def test_the_entry_point_is_declared_exported_and_bound(built):
    HS.declared_exported_bound(
        "rtggx_set_light_reflections", r"\bint\s+rtggx_set_light_reflections\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*int\s+enable\s*\)",
        defines=(r"\bRTGGX_BUF_COUNT\s*=\s*28\b", r"rtggx_set_light_reflections\(ctx, 1\) lifts the limit",
                 r"j = 32 \+ 16 d \+ 8 img \+ i", r"so 32 \.\. 95 collide with neither", r"F: the frame's FrameIndex at one sample; for sample k of an N-sample frame FrameIndex N \+ k",
                 r"term_c = \(F_c k\) \(I_c att\)", r"g = \(NoL / pi\) att; term_c = \(color'_c g\) I_c", r"s = T_d term, per component",
                 r"first the sun's s_d \(where that feature is active and has a term\), then the lights' terms for i ascending",
                 r"one rounding whichever features are on", r"both bounds exclusive, skipping the hit's \(inst, prim\), through the any-hit traversal",
                 r"With rho = 0 there is no hash, and Ls and L are the same bits", r"56 \+ 8 \+ 8 bytes per ray slot"))
    from raytracedggx_amd import app, capi
    assert capi.load().rtggx_set_light_reflections.argtypes == [C.c_void_p, C.c_int]
    assert "rtggx_app_set_light_reflections" in app.HOST_EXPORTS and hasattr(C.CDLL(app.HOST_LIB_PATH), "rtggx_app_set_light_reflections")
    assert callable(getattr(app.RayTracedGGX, "set_light_reflections", None))
    for name in ("RayTracedGGX.h", "RayTracedGGX.cpp"):      # the flag list and kFlags
        text = open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", name)).read()
        assert "-lightreflections" in text or '"lightreflections"' in text
    assert "SetLightReflections" in open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", "RayTracer.h")).read()


POINT = ["-light", "1", "2", "3", "4", "5", "6", "7"]
SPOT = ["-spot", "1", "2", "3", "4", "5", "6", "9", "0.5", "0", "-1", "0", "30", "20"]


def test_the_executable_refuses_the_flag_without_lights_before_asking_for_a_device(built):
    HS.executable_refuses([
        (["-lightreflections"], "-lightreflections"), (["-lightreflections", "-rayrate", "4"], "-lightreflections"),
        (["-sun", "0", "1", "0", "1", "1", "1", "-sunreflections", "-lightreflections"], "-lightreflections"),
        (["-lightreflections"] + POINT + ["-rayrate", "4"], "-rayrate 4"), (SPOT + ["-rayrate", "4", "-lightreflections"], "-rayrate 4")])


def test_the_executable_parses_the_flag_with_lights(built, tmp_path):
    """What stops these runs is the environment file, which is read after the command line and before a device is asked for."""
    import assets
    missing = str(tmp_path / "missing.hdr")
    HS.executable_refuses([["-env", missing, "-lightreflections"] + POINT, ["-env", missing] + SPOT + ["-lightreflections"],
                           ["-env", missing] + POINT + ["-lightreflections"] + SPOT + ["-sun", "0", "1", "0", "1", "1", "1", "-sunreflections", "-recursion", "2"]],
                          must_mention="cannot open", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def frame(cls, size, lights=None, sun=False, depth=1, samples=1, metallic=MIXED, toggle=None, force_walker=False):
    o = cls(size[0], size[1], depth=depth, samples=samples)
    try:
        HS.scene(o, metallic=metallic)
        if sun:
            o.set_sun(*SUN); o.set_sun_reflections(True); o.set_sun_angle(5.0)
        if lights is not None:
            o.set_lights(lights)
        if toggle is not None:
            o.set_light_reflections(toggle)
            o.force_walker = force_walker
        rays = o.ray_trace()
        out = dict(refl=o.buffer(O.BUF_RT_REFL), diff=o.buffer(O.BUF_RT_DIFF), rays=rays, classes=o.classes.copy(), light_classes=o.light_classes.copy())
        if toggle is not None:
            out.update(hit_rays=o.light_hit_rays, light_lit=o.light_lit.copy(), counts=o.light_counts.copy())
        return out
    finally:
        o.close()


ZERO = [dict(position=[0, 5, 0], intensity=[0, 0, 0], range=30.0), dict(position=[-8, 0.3, -6], intensity=[0, 0, 0], range=25.0, radius=0.5)]


@pytest.mark.parametrize("sun", [False, True], ids=["no sun", "behind the sun's passes"])
@pytest.mark.parametrize("samples", [1, 2], ids=["N = 1", "N = 2"])
@pytest.mark.parametrize("depth", [1, 2], ids=["D = 1", "D = 2"])
def test_without_the_toggle_or_lights_the_frame_is_lights_refs(sun, depth, samples):
    """The copied walker has not drifted: with the toggle off (the walker forced), with no lights and with lights that cast no ray the frame,
    the sun's classes, the lights' classes and the ray count are lights_ref's, and no shadow ray leaves a hit."""
    kw = dict(sun=sun, depth=depth, samples=samples)
    for lights, toggle, forced in ((LIGHTS, 0, True), (None, 1, True), ([], 1, False), (ZERO, 1, False), (ZERO, 1, True)):
        want = frame(LR.Oracle, SMALL, lights=lights, **kw)
        got = frame(LH.Oracle, SMALL, lights=lights, toggle=toggle, force_walker=forced, **kw)
        for k in want:
            assert np.array_equal(got[k], want[k]), (lights is LIGHTS, toggle, forced, k)
        assert got["hit_rays"] == 0 and not got["light_lit"].any() and not got["counts"].any()


def fields(words):
    """The three unsigned small floats of R11G11B10F words as integers: ordered as their values are."""
    w = words.astype(np.uint32)
    return np.stack([w & 0x7FF, (w >> 11) & 0x7FF, w >> 22])


@pytest.mark.parametrize("sun,depth,samples", [(False, 1, 1), (True, 2, 1), (False, 2, 2)], ids=["D = 1", "the sun, D = 2", "D = 2, N = 2"])
def test_with_the_toggle_words_only_grow_and_only_where_a_lit_hit_was_recorded(sun, depth, samples):
    kw = dict(sun=sun, depth=depth, samples=samples)
    off = frame(LR.Oracle, (W, H), lights=LIGHTS, **kw)
    on = frame(LH.Oracle, (W, H), lights=LIGHTS, toggle=1, **kw)
    for bit, k in ((1, "refl"), (2, "diff")):
        a, b = fields(off[k]), fields(on[k])
        assert (b >= a).all(), k
        changed = (off[k] != on[k])
        assert changed.any() and not (changed & ((on["light_lit"] & bit) == 0)).any(), k
    assert on["hit_rays"] > 0 and on["rays"] == off["rays"] + on["hit_rays"]
    c = on["counts"]
    assert on["hit_rays"] == int(c[..., LH.COLUMNS.index("occluded")].sum() + c[..., LH.COLUMNS.index("lit")].sum())
    assert np.array_equal(c[..., LH.COLUMNS.index("lit")], c[..., LH.COLUMNS.index("lit_specular")] + c[..., LH.COLUMNS.index("lit_diffuse")])
    assert not c[depth:].any() and c[depth - 1].any()
    assert np.array_equal(on["classes"], off["classes"]) and np.array_equal(on["light_classes"], off["light_classes"])      # (the primary passes)


def test_all_metal_materials_leave_the_second_image_alone():
    off = frame(LR.Oracle, (W, H), lights=LIGHTS, depth=2, metallic=(1.0, 1.0))
    on = frame(LH.Oracle, (W, H), lights=LIGHTS, depth=2, metallic=(1.0, 1.0), toggle=1)
    assert np.array_equal(on["diff"], off["diff"]) and not (on["light_lit"] & 2).any()
    assert (on["refl"] != off["refl"]).any() and not on["counts"][..., LH.COLUMNS.index("lit_diffuse")].any()


def test_the_restatement_refuses_other_values():
    o = LH.Oracle(16, 16)
    try:
        o.set_light_reflections(1)
        for bad in (2, -1, 256):
            with pytest.raises(ValueError):
                o.set_light_reflections(bad)
        assert o.light_reflections
    finally:
        o.close()


# ---- the hash slots -----------------------------------------------------------------------------------------------------------------------
def test_the_hash_slots_worked_out_by_hand():
    """(pixel, frame index, level, image, light) -> (w, u 65536, s) from Python integers against the restatement's; the 64 slots are distinct
    and meet neither the sun's 0 .. 8 nor the primary lights' 16 .. 23."""
    slots = {LH.slot(d, img, i) for d in range(4) for img in range(2) for i in range(8)}
    assert len(slots) == 64 and min(slots) == 32 and max(slots) == 95
    assert not slots & (set(range(0, 9)) | set(range(16, 24)))
    assert LH.slot(0, 0, 0) == 32 and LH.slot(1, 0, 2) == 50 and LH.slot(3, 1, 7) == 95
    seen = set()
    for case in ((0, 0, 0, 0, 0), (1, 0, 0, 1, 0), (5, 7, 1, 0, 2), (12431, 1, 3, 1, 7), (2073599, 4000000000, 2, 1, 3), (77, 12345, 0, 1, 1)):
        want = LH.sample_words(*case)
        assert want == LH.sample_words_lib(*case), case
        seen.add(want)
    assert len(seen) == 6
    # the slot is the only thing that tells the levels, images and lights of one pixel and frame apart; and no slot draws a primary light's word
    own = {LH.sample_words(7, 3, d, img, i) for d in range(4) for img in range(2) for i in range(8)}
    primary = {(u, s) for (_, u, s) in (LR.sphere_sample(7, 3, i) for i in range(8))}
    assert len(own) == 64 and not {(u / 65536.0, s) for (_, u, s) in own} & primary


# ---- the class conditions of the scene the GPU tests use ---------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2], ids=["depth 1", "depth 2"])
def test_the_class_conditions_of_the_scene_the_gpu_tests_use(depth):
    """lights_classes.json's scene and lights A, B and C over the first FRAMES frame indices of the still scene: the conditions hold on the
    restatement alone, and the counts are the golden file's."""
    assert {k: GOLDEN[k] for k in ("width", "height", "metallic", "lights", "spot_degrees")} == {
        k: json.load(open(os.path.join(HS.ROOT, "tests", "golden", "lights_classes.json")))[k] for k in ("width", "height", "metallic", "lights", "spot_degrees")}
    assert GOLDEN["columns"] == list(LH.COLUMNS)
    o = LH.Oracle(W, H, depth=depth)
    try:
        HS.scene(o, metallic=MIXED)
        base = HS.frame_index(o)
        o.set_lights(LIGHTS); o.set_light_reflections(1)
        frames = []
        for f in range(FRAMES):
            HS.set_frame_index(o, base + f)
            o.ray_trace()
            frames.append((o.light_counts.copy(), o.light_cls0.copy(), o.light_hit_rays))
        got = LH.figures(frames, len(LIGHTS))
        assert got == GOLDEN["depth%d" % depth], got
        LH.check_conditions(got, RADII, "golden, depth %d" % depth, depth)
    finally:
        o.close()
