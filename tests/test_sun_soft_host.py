"""A sun with a size, the part that needs no GPU: rtggx_set_sun_angle declared, exported and bound; -sunangle checked at parse time; the
restatement (tests/sun_soft_ref.cpp) against tests/sun_hit_ref.cpp's frames at angle 0; what an angle may change, against the angle-0 twin of
the same frame; the geometry of the samples; and the class conditions of the scene the GPU tests use (tests/golden/sun_soft_classes.json)."""
import json
import math
import os

import numpy as np
import pytest

import host_support as HS
import sun_hit_ref as SH
import sun_ref as SR
import sun_soft_ref as SS
from oracle import oracle as O

GOLDEN = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "sun_soft_classes.json")))
L, E = GOLDEN["direction"], GOLDEN["irradiance"]
W, H = GOLDEN["width"], GOLDEN["height"]
MIXED = tuple(GOLDEN["metallic"])
ANGLE = GOLDEN["angle"]
FRAMES = GOLDEN["frames"]


def test_the_entry_point_is_declared_exported_and_bound(built):
    HS.declared_exported_bound(
        "rtggx_set_sun_angle", r"\bint\s+rtggx_set_sun_angle\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*float\s+degrees\s*\)",
        defines=(r"#define\s+RTGGX_MAX_SUN_ANGLE_DEGREES\s+10\.0f", r"\bRTGGX_BUF_COUNT\s*=\s*28\b", r"evaluated at the centre direction"))
    from raytracedggx_amd import capi
    assert capi.MAX_SUN_ANGLE_DEGREES == SS.MAX_ANGLE == 10.0
    for name in ("RayTracedGGX.h", "RayTracedGGX.cpp"):      # the flag list and kFlags
        assert "sunangle" in open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", name)).read()


SUN = ["-sun"] + [str(x) for x in L + E]


def test_the_executable_refuses_bad_angles_before_asking_for_a_device(built):
    HS.executable_refuses([SUN + ["-sunangle"], SUN + ["-sunangle", "nan"], SUN + ["-sunangle", "-1"], SUN + ["-sunangle", "10.5"], SUN + ["-sunangle", "4x"],
                           ["-sunangle", "4x", "-sunfromenv"], ["-sunangle", "2"], ["-sunangle", "2", "-recursion", "2"]], must_mention="-sunangle")


def test_the_executable_parses_an_angle_with_either_sun(built, tmp_path):
    """What stops these runs is the environment file, which is read after the command line and before a device is asked for."""
    missing = str(tmp_path / "missing.hdr")
    import assets
    HS.executable_refuses([["-sunangle", "2", "-sunfromenv", "-env", missing], ["-env", missing, "-sunangle", "0"] + SUN, ["-env", missing] + SUN + ["-sunangle", "10"],
                           ["-env", missing, "-sunfromenv", "6", "-sunangle", "0.27", "-sunreflections"]],
                          must_mention="cannot open", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def frame(cls, depth=1, samples=1, sun=(L, E), reflections=False, angle=None, index=None, statistics=False, force_rule=False):
    """One frame of `cls` on the golden scene: the words, the ray count and (sun_soft_ref's Oracle) its records."""
    o = cls(W, H, depth=depth, samples=samples)
    try:
        HS.scene(o, metallic=MIXED)
        if index is not None:
            HS.set_frame_index(o, index)
        if sun is not None:
            o.set_sun(*sun)
        o.set_sun_reflections(reflections)
        if angle is not None:
            o.set_sun_angle(angle); o.statistics = statistics; o.force_rule = force_rule
        rays = o.ray_trace()
        rec = dict(refl=o.buffer(O.BUF_RT_REFL), diff=o.buffer(O.BUF_RT_DIFF), rays=rays, classes=o.classes.copy(), counts=o.counts.copy(), lit=o.lit.copy())
        if cls is SS.Oracle:
            rec.update(centre=o.centre.copy(), changed=o.changed.copy(), soft=o.soft.copy())
        return rec
    finally:
        o.close()


CASES = [(1, 1), (2, 1), (1, 2), (2, 2)]


@pytest.mark.parametrize("reflections", [False, True], ids=["toggle off", "toggle on"])
@pytest.mark.parametrize("depth,samples", CASES)
def test_at_angle_0_the_frame_is_sun_hit_refs(depth, samples, reflections):
    """Through the new functions with k = 0 (force_rule: sun_soft_pixel, follow_path_s, raygen_pixel_s -- the rule gives Ls = L exactly), with
    and without their statistics, and through the hand-over an Oracle at angle 0 takes."""
    want = frame(SH.Oracle, depth, samples, reflections=reflections)
    for angle, force, statistics in ((0.0, True, False), (0.0, True, True), (None, False, False), (0.0, False, False)):
        got = frame(SS.Oracle, depth, samples, reflections=reflections, angle=angle, force_rule=force, statistics=statistics)
        for k in ("refl", "diff", "rays", "classes", "counts", "lit"):
            assert np.array_equal(got[k], want[k]), (angle, force, k)
        assert not got["soft"].any() and not got["changed"].any()
        assert not statistics or np.array_equal(got["centre"], want["classes"])


@pytest.fixture(scope="module")
def twins():
    """By (depth, samples, toggle): the frame at the golden angle with its statistics, the directional sun's, the sunless one, and the
    directional sun's words where nothing occludes it."""
    out = {}
    for depth, samples, reflections in ((1, 1, False), (2, 1, True), (2, 2, True)):
        soft = frame(SS.Oracle, depth, samples, reflections=reflections, angle=ANGLE, statistics=True)
        hard = frame(SS.Oracle, depth, samples, reflections=reflections, angle=0.0)
        none = frame(SS.Oracle, depth, samples, sun=None)
        o = SS.Oracle(W, H, depth=depth, samples=samples)
        try:
            HS.scene(o, metallic=MIXED)
            o.ray_trace()
            o.set_sun(L, E)
            lit = o.lit_words()
        finally:
            o.close()
        out[(depth, samples, reflections)] = (soft, hard, none, lit)
    return out


@pytest.mark.parametrize("key", [(1, 1, False), (2, 1, True), (2, 2, True)], ids=["depth 1", "depth 2 with reflections", "depth 2, N = 2, with reflections"])
def test_words_differ_from_the_directional_suns_only_where_a_sampled_ray_ends_otherwise(twins, key):
    soft, hard, none, lit = twins[key]
    primary = soft["classes"] != soft["centre"]
    assert np.array_equal(soft["centre"], hard["classes"])
    assert primary.any()
    for bit, name in ((1, "refl"), (2, "diff")):
        may = primary | ((soft["changed"] & bit) != 0)
        assert np.array_equal(soft[name][~may], hard[name][~may]), name
        assert (soft[name][may] != hard[name][may]).any(), name
    if not key[2]:      # the primary pass alone: the two words a pixel can carry
        went_dark = (soft["centre"] == SS.LIT) & (soft["classes"] != SS.LIT)
        went_lit = (soft["centre"] == SS.OCCLUDED) & (soft["classes"] == SS.LIT)
        assert went_dark.sum() >= 20 and went_lit.sum() >= 20, (int(went_dark.sum()), int(went_lit.sum()))
        assert (soft["classes"][went_dark] == SS.BELOW_HORIZON).any() and (soft["classes"][went_dark] == SS.OCCLUDED).any()
        for name, words in (("refl", 0), ("diff", 1)):
            assert np.array_equal(soft[name][went_dark], none[name][went_dark]), name
            assert np.array_equal(soft[name][went_lit], lit[words][went_lit]), name
        lit_both = (soft["centre"] == SS.LIT) & (soft["classes"] == SS.LIT)
        assert np.array_equal(hard["refl"][lit_both], lit[0][lit_both])      # (the aid is the directional sun's lit word)
        # rays: one per sun-facing pixel above the horizon
        assert soft["rays"] == hard["rays"] - int((soft["classes"] == SS.BELOW_HORIZON).sum())
    else:
        assert soft["soft"][:, SS.SOFT_COLUMNS.index("differs")].sum() > 0 and soft["soft"][:, SS.SOFT_COLUMNS.index("below_horizon")].sum() > 0


# ---- the geometry of the samples ---------------------------------------------------------------------------------------------------------
def test_the_disk_frame_is_orthonormal_and_the_samples_fill_the_cap():
    for direction in (L, (0.0, 1.0, 0.0), (1.0, 1.0, 1.0), (0.3, -0.3, 0.9), (-2.0, 0.0, 0.0)):
        l = SR.normalise(direction)
        k, t, b = SS.disk(l, 5.0)
        m = np.stack([t, b, l]).astype(np.float64)
        assert np.abs(m @ m.T - np.eye(3)).max() <= 2e-7, direction
        assert np.abs(np.cross(t.astype(np.float64), b.astype(np.float64)) - l).max() <= 4e-7      # right-handed: T x B = L
        assert abs(float(k) - (1.0 - math.cos(math.radians(5.0)))) <= 2.0 ** -24 * 0.0039
    l = SR.normalise(L)
    us, slots = [], set()
    for frame_index in range(64):
        for pixel in range(64):
            ls, u, s = SS.sample(pixel, frame_index, 0, l, 5.0)
            ls = ls.astype(np.float64)
            assert ls @ l.astype(np.float64) >= math.cos(math.radians(5.0)) - 4e-7
            assert abs(math.sqrt(ls @ ls) - 1.0) <= 4e-7
            us.append(u); slots.add(s)
    assert len(slots) == 256
    assert abs(np.mean(us) - 0.5) <= 0.03      # sigma of a mean of 4096 uniforms: 0.0045
    # the slots of one pixel and frame are different draws
    assert len({SS.sample(7, 3, j, l, 5.0)[1:] for j in range(9)}) == 9
    # a small disk: sin(theta) from e (2 - e) keeps its digits where 1 - cos^2 has lost them
    ls, u, s = SS.sample(11, 5, 0, l, 0.25)
    k = float(SS.disk(l, 0.25)[0])
    off = ls.astype(np.float64) - l.astype(np.float64) * (1.0 - u * k)
    assert abs(math.sqrt(off @ off) - math.sqrt(u * k * (2.0 - u * k))) <= 1e-3 * math.sqrt(u * k * (2.0 - u * k)) + 1e-7


# (pixel, FrameIndex, j) -> (w, w & 0xffff, w >> 24): steps 1-3 of the header's rule worked out apart from the restatement, with Python
# integers (rng is RayTracing.hlsl's: x = x 747796405 + 1; x = ((x >> ((x >> 28) + 4)) ^ x) 277803737; x = (x >> 22) ^ x, all mod 2^32)
VECTORS = (((0, 0, 0), (0xF37A5CE3, 23779, 243)), ((1, 0, 0), (0x159A215B, 8539, 21)), ((5, 7, 0), (0xB90CA488, 42120, 185)),
           ((12431, 1, 3), (0xB82C06CC, 1740, 184)), ((2073599, 4000000000, 8), (0xE6AF62EC, 25324, 230)), ((77, 12345, 1), (0xF9BD0555, 1365, 249)))


def _rng(x):
    x = (x * 747796405 + 1) & 0xFFFFFFFF
    x = (((x >> ((x >> 28) + 4)) ^ x) * 277803737) & 0xFFFFFFFF
    return ((x >> 22) ^ x) & 0xFFFFFFFF


def test_the_restated_direction_equals_the_rule_worked_out_by_hand():
    """The words above are what this file's own integer arithmetic gives; u and s of the restatement are their low 16 and high 8 bits; and Ls
    is steps 4 and 5 in numpy's float32, one rounded operation at a time, bit for bit."""
    f = np.float32
    l = SR.normalise(L)
    for angle in (5.0, 0.25):
        k, t, b = SS.disk(l, angle)
        table = [(f(math.cos(2.0 * 3.14159265358979323846 * s / 256.0)), f(math.sin(2.0 * 3.14159265358979323846 * s / 256.0))) for s in range(256)]
        for (pixel, index, j), (w, low, high) in VECTORS:
            assert _rng((_rng((_rng(pixel) + index) & 0xFFFFFFFF) + j * 0x9E3779B9) & 0xFFFFFFFF) == w and (w & 0xFFFF, w >> 24) == (low, high)
            ls, u, s = SS.sample(pixel, index, j, l, angle)
            assert (u, s) == (low / 65536.0, high), (pixel, index, j)
            e = f(u) * k
            cos_t, sin_t = f(1.0) - e, np.sqrt(e * (f(2.0) - e), dtype=np.float32)
            ct, st = table[s][0] * sin_t, table[s][1] * sin_t
            want = np.array([(t[c] * ct + b[c] * st) + l[c] * cos_t for c in range(3)], np.float32)
            assert np.array_equal(want.view(np.uint32), ls.view(np.uint32)), (pixel, index, j, angle)


# ---- the class conditions of the scene the GPU tests use ---------------------------------------------------------------------------------
def test_the_class_conditions_of_the_scene_the_gpu_tests_use():
    """Over the first FRAMES frame indices of the still scene at the golden angle: pixels that are lit in one frame and occluded in another,
    pixels with a sample below the horizon, and -- depth 2 with the toggle on -- hits below the horizon and hits whose sampled ray ends
    otherwise than the centre ray.  The counts are the golden file's; the bars are the ones the GPU tests assert again on their own frames."""
    o = SS.Oracle(W, H, depth=2)
    try:
        HS.scene(o, metallic=MIXED)
        base = HS.frame_index(o)
        o.set_sun(L, E); o.set_sun_reflections(True); o.set_sun_angle(ANGLE); o.statistics = True
        classes, soft = [], np.zeros_like(o.soft)
        for f in range(FRAMES):
            HS.set_frame_index(o, base + f)
            o.ray_trace()
            classes.append(o.classes.copy()); soft += o.soft
        classes = np.stack(classes)
        facing = int((o.centre >= SS.OCCLUDED).sum())
        mixed = int(((classes == SS.LIT).any(0) & (classes == SS.OCCLUDED).any(0)).sum())
        below = int((classes == SS.BELOW_HORIZON).any(0).sum())
        got = dict(sun_facing=facing, mixed=mixed, below_horizon=below,
                   hits_below_horizon=[int(x) for x in soft[:2, 0]], hits_differ=[int(x) for x in soft[:2, 1]])
        assert got == {k: GOLDEN[k] for k in got}, got
        assert mixed >= 100 and below >= 20
        assert sum(got["hits_below_horizon"]) >= 20 and sum(got["hits_differ"]) >= 20
    finally:
        o.close()
