"""Local lights, the part that needs no GPU: rtggx_set_lights declared, exported and bound; capi.Light's layout; -light and -spot checked at
parse time; the restatement (tests/lights_ref.cpp) against tests/sun_soft_ref.cpp's frames without lights; what it refuses; the points of
the emitting sphere; the hash slots worked out apart from it; and the class conditions of the scene the GPU tests use
(tests/golden/lights_classes.json)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import host_support as HS
import lights_ref as LR
import sun_soft_ref as SS
from oracle import oracle as O

GOLDEN = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "lights_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]
FRAMES = GOLDEN["frames"]
SUN = ([-0.6, 0.5, -0.3], [3.0, 3.0, 3.0])


def test_the_entry_point_is_declared_exported_and_bound(built):
    HS.declared_exported_bound(
        "rtggx_set_lights", r"\bint\s+rtggx_set_lights\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*const\s+RtggxLight\s*\*\s*lights\s*,\s*uint32_t\s+count\s*\)",
        defines=(r"#define\s+RTGGX_MAX_LIGHTS\s+8u", r"\bRTGGX_BUF_COUNT\s*=\s*28\b", r"typedef\s+struct\s+RtggxLight\s*\{\s*/\*\s*64 bytes\s*\*/",
                 r"surfaces seen in reflections get no light term", r"evaluated at the centre direction L \(only visibility is sampled"))
    from raytracedggx_amd import app, capi
    assert C.sizeof(capi.Light) == 64 and capi.MAX_LIGHTS == LR.MAX_LIGHTS == 8
    assert [n for n, _ in capi.Light._fields_] == ["position", "range", "intensity", "radius", "axis", "cos_outer", "cos_inner", "pad"]
    assert (capi.Light.range.offset, capi.Light.radius.offset, capi.Light.cos_outer.offset, capi.Light.cos_inner.offset) == (12, 28, 44, 48)
    l = capi.Light.of(**LIGHTS[1])
    assert np.array_equal(np.frombuffer(bytes(l), np.float32)[:13], np.float32(LIGHTS[1]["position"] + [LIGHTS[1]["range"]] + LIGHTS[1]["intensity"]
                          + [LIGHTS[1]["radius"]] + LIGHTS[1]["axis"] + [LIGHTS[1]["cos_outer"], LIGHTS[1]["cos_inner"]]))
    assert "rtggx_app_set_lights" in app.HOST_EXPORTS and hasattr(C.CDLL(app.HOST_LIB_PATH), "rtggx_app_set_lights")
    assert callable(getattr(app.RayTracedGGX, "set_lights", None))
    for name in ("RayTracedGGX.h", "RayTracedGGX.cpp"):      # the flag list and kFlags
        text = open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", name)).read()
        assert "-light" in text or '"light"' in text
        assert "-spot" in text or '"spot"' in text
    assert "SetLights" in open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", "RayTracer.h")).read()


POINT = ["-light", "1", "2", "3", "4", "5", "6", "7"]
SPOT = ["-spot", "1", "2", "3", "4", "5", "6", "9", "0.5", "0", "-1", "0", "30", "20"]


def test_the_executable_refuses_bad_lights_before_asking_for_a_device(built):
    nine = POINT * 5 + SPOT * 4
    HS.executable_refuses([
        (["-light"], "-light"), (POINT[:7], "-light"), (POINT[:4] + ["x"] + POINT[5:], "-light"), (POINT[:1] + ["nan"] + POINT[2:], "-light"),
        (POINT[:4] + ["-1"] + POINT[5:], "-light"), (POINT[:4] + ["inf"] + POINT[5:], "-light"),
        (POINT[:7] + ["0"], "-light"), (POINT[:7] + ["-2"], "-light"), (POINT[:7] + ["inf"], "-light"),      # the range
        (POINT + ["-0.1"], "-light"), (POINT + ["7"], "-light"), (POINT + ["8"], "-light"), (POINT + ["nan"], "-light"),      # the radius
        (SPOT[:13], "-spot"), (SPOT[:9] + ["0", "0", "0"] + SPOT[12:], "-spot"), (SPOT[:9] + ["nan"] + SPOT[10:], "-spot"),
        (SPOT[:12] + ["20", "30"], "-spot"), (SPOT[:12] + ["30", "30"], "-spot"), (SPOT[:12] + ["180", "20"], "-spot"), (SPOT[:12] + ["30", "0"], "-spot"),
        (SPOT[:12] + ["nan", "20"], "-spot"), (SPOT[:8] + ["9"] + SPOT[9:], "-spot"),
        (nine, "at most 8 lights"), (POINT + ["-rayrate", "4"], "-rayrate 4"), (["-rayrate", "4"] + SPOT, "-rayrate 4")])


def test_the_executable_parses_good_lights(built, tmp_path):
    """What stops these runs is the environment file, which is read after the command line and before a device is asked for."""
    import assets
    missing = str(tmp_path / "missing.hdr")
    HS.executable_refuses([["-env", missing] + POINT, ["-env", missing] + POINT + ["0.5"] + SPOT, ["-env", missing] + POINT * 4 + SPOT * 4,
                           ["-env", missing] + SPOT + ["-sun", "0", "1", "0", "1", "1", "1", "-recursion", "2"]],
                          must_mention="cannot open", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def frame(cls, lights=None, sun=None, depth=1, samples=1):
    o = cls(W, H, depth=depth, samples=samples)
    try:
        HS.scene(o, metallic=MIXED)
        if sun:
            o.set_sun(*SUN); o.set_sun_reflections(True); o.set_sun_angle(5.0)
        if lights is not None:
            o.set_lights(lights)
        rays = o.ray_trace()
        return dict(refl=o.buffer(O.BUF_RT_REFL), diff=o.buffer(O.BUF_RT_DIFF), rays=rays, classes=o.classes.copy())
    finally:
        o.close()


@pytest.mark.parametrize("sun,depth,samples", [(False, 1, 1), (True, 2, 1), (True, 1, 2)], ids=["no sun", "the sun, depth 2", "the sun, N = 2"])
def test_without_lights_the_frame_is_sun_soft_refs(sun, depth, samples):
    want = frame(SS.Oracle, sun=sun, depth=depth, samples=samples)
    for lights in (None, [], [dict(position=[0, 5, 0], intensity=[0, 0, 0], range=30.0)]):      # never set, count == 0, a light that casts no ray
        got = frame(LR.Oracle, lights=lights, sun=sun, depth=depth, samples=samples)
        for k in want:
            assert np.array_equal(got[k], want[k]), (lights, k)
    lit = frame(LR.Oracle, lights=LIGHTS, sun=sun, depth=depth, samples=samples)
    assert (lit["refl"] != want["refl"]).any() and (lit["diff"] != want["diff"]).any() and lit["rays"] > want["rays"]
    assert np.array_equal(lit["classes"], want["classes"])      # (the sun's classes)


def test_the_restatement_refuses_what_the_product_refuses():
    ok = dict(position=[0.0, 5.0, 0.0], intensity=[1.0, 1.0, 1.0], range=10.0)
    nan, inf = float("nan"), float("inf")
    LR.records([ok] * 8)
    LR.record(**dict(ok, radius=9.99)); LR.record(**dict(ok, axis=[0, 0, 0])); LR.record(**dict(ok, cos_outer=-2.0, axis=[nan, 0, 0]))
    LR.record(**dict(ok, axis=[0, -1, 0], cos_outer=0.5, cos_inner=1.0))
    with pytest.raises(ValueError):
        LR.records([ok] * 9)
    for bad in (dict(position=[nan, 0, 0]), dict(position=[0, inf, 0]), dict(range=0.0), dict(range=-1.0), dict(range=inf), dict(range=nan),
                dict(intensity=[1, -1e-9, 1]), dict(intensity=[inf, 0, 0]), dict(intensity=[0, 0, nan]), dict(radius=-0.1), dict(radius=10.0), dict(radius=nan),
                dict(radius=inf), dict(cos_outer=0.5, cos_inner=0.9), dict(cos_outer=0.5, cos_inner=0.9, axis=[0, inf, 0]), dict(cos_outer=0.5, cos_inner=0.9, axis=[nan, 1, 0]),
                dict(axis=[0, 1, 0], cos_outer=0.5, cos_inner=0.5), dict(axis=[0, 1, 0], cos_outer=0.9, cos_inner=0.5), dict(axis=[0, 1, 0], cos_outer=0.5, cos_inner=1.5),
                dict(axis=[0, 1, 0], cos_outer=nan, cos_inner=0.5), dict(axis=[0, 1, 0], cos_outer=0.5, cos_inner=nan)):
        with pytest.raises(ValueError):
            LR.record(**dict(ok, **bad))
    f = LR.record(**dict(ok, axis=[3.0, -4.0, 12.0], cos_outer=0.5, cos_inner=0.9))      # the axis: double, rounded once
    assert np.array_equal(f[8:11], (np.array([3.0, -4.0, 12.0]) / 13.0).astype(np.float32))


# ---- the points of the sphere ------------------------------------------------------------------------------------------------------------
def test_every_point_of_the_sphere_has_length_1():
    """All 65 536 values of u and 256 of s: |o| within 1e-6 of 1 (the lengths in double, on the fp32 components)."""
    out = np.zeros(2, np.float32)
    LR.lib().orc_light_sphere_points(LR._p(out))
    print("|o| - 1 over all (u, s): %.3e .. %.3e" % (out[0], out[1]))
    assert -1e-6 <= out[0] <= out[1] <= 1e-6
    o = np.zeros(3, np.float32)
    for k, want_z in ((0, 1.0), (32768, 0.0), (65535, -1.0 + 2.0 / 65536.0)):      # z = 1 - 2 u is exact
        LR.lib().orc_light_sphere_point(k, 0, LR._p(o))
        assert float(o[2]) == want_z and o[1] == 0.0


def _rng(x):
    x = (x * 747796405 + 1) & 0xFFFFFFFF
    x = (((x >> ((x >> 28) + 4)) ^ x) * 277803737) & 0xFFFFFFFF
    return ((x >> 22) ^ x) & 0xFFFFFFFF


def test_the_restated_point_equals_the_rule_worked_out_by_hand():
    """Step 5 with Python integers and numpy's float32, one rounded operation at a time: the slots start at 16, and a light keeps its own."""
    f = np.float32
    table = [(f(math.cos(2.0 * 3.14159265358979323846 * s / 256.0)), f(math.sin(2.0 * 3.14159265358979323846 * s / 256.0))) for s in range(256)]
    seen = set()
    for pixel, index, i in ((0, 0, 0), (1, 0, 0), (5, 7, 2), (12431, 1, 7), (2073599, 4000000000, 3), (77, 12345, 1)):
        w = _rng((_rng((_rng(pixel) + index) & 0xFFFFFFFF) + (16 + i) * 0x9E3779B9) & 0xFFFFFFFF)
        o, u, s = LR.sphere_sample(pixel, index, i)
        assert (u, s) == ((w & 0xFFFF) / 65536.0, w >> 24), (pixel, index, i)
        z = f(1.0) - f(2.0) * f(u)
        rho = np.sqrt(f(1.0) - z * z, dtype=np.float32)
        want = np.array([rho * table[s][0], rho * table[s][1], z], np.float32)
        assert np.array_equal(want.view(np.uint32), o.view(np.uint32)), (pixel, index, i)
        seen.add((u, s))
    assert len(seen) == 6
    assert len({LR.sphere_sample(7, 3, i)[1:] for i in range(8)} | {SS.sample(7, 3, j, np.float32([0, 1, 0]), 5.0)[1:] for j in range(9)}) == 17      # no slot of the sun's


# ---- the class conditions of the scene the GPU tests use ---------------------------------------------------------------------------------
def test_the_class_conditions_of_the_scene_the_gpu_tests_use():
    """The three lights -- A, a point light whose range ends on the ground; B, a spot with a radius whose cone edge and bunny shadow fall on
    the ground; C, a low light with a radius -- over the first FRAMES frame indices of the still scene.  The counts are the golden file's."""
    assert LIGHTS[0].get("radius", 0.0) == 0.0 and "cos_outer" not in LIGHTS[0] and LIGHTS[1]["radius"] > 0 and LIGHTS[2]["radius"] > 0
    assert (LIGHTS[1]["cos_outer"], LIGHTS[1]["cos_inner"]) == LR.cone(*GOLDEN["spot_degrees"])
    o = LR.Oracle(W, H)
    try:
        HS.scene(o, metallic=MIXED)
        base = HS.frame_index(o)
        o.set_lights(LIGHTS); o.statistics_lights = True
        classes, aux, rays = [], [], []
        for f in range(FRAMES):
            HS.set_frame_index(o, base + f)
            total = o.ray_trace()
            classes.append(o.light_classes.copy()); aux.append(o.light_aux.copy()); rays.append(o.light_rays)
            assert total > o.light_rays > 0
        got = LR.figures(np.stack(classes), np.stack(aux))
        assert got["light_rays"] == rays
        assert got == {k: GOLDEN[k] for k in got}, got
        LR.check_conditions(got, "golden")
        # with every radius 0 no light has a pixel below the horizon, and the frame does not depend on the frame index
        o.set_lights([dict(l, radius=0.0) for l in LIGHTS])
        words = []
        for f in range(2):
            HS.set_frame_index(o, base + f)
            HS.poison(o)
            o.ray_trace()
            assert not (o.light_classes == LR.BELOW_HORIZON).any()
            words.append((o.light_classes.copy(), o.light_rays))
        assert np.array_equal(words[0][0], words[1][0]) and words[0][1] == words[1][1]
    finally:
        o.close()
