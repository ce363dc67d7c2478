"""The sun at the surfaces the paths hit, the part that needs no GPU: rtggx_set_sun_reflections declared, exported and bound; -sunreflections
without -sun refused at parse time; the restatement (tests/sun_hit_ref.cpp) against tests/sun_ref.cpp's frame with the toggle off and against
the stock oracle without irradiance; what the toggle may change; the ray count; and the class shares of the scene the GPU tests use
(tests/golden/sun_hit_classes.json)."""
import json
import os

import numpy as np
import pytest

import host_support as HS
import sun_hit_ref as SH
import sun_ref as SR
from oracle import oracle as O

GOLDEN = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "sun_hit_classes.json")))
L, E = GOLDEN["direction"], GOLDEN["irradiance"]
W, H = GOLDEN["width"], GOLDEN["height"]
MIXED = tuple(GOLDEN["metallic"])


def test_the_entry_point_is_declared_exported_and_bound(built):
    HS.declared_exported_bound(
        "rtggx_set_sun_reflections", r"\bint\s+rtggx_set_sun_reflections\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*int\s+enable\s*\)",
        defines=(r"\bRTGGX_BUF_COUNT\s*=\s*28\b", r"Known limit: surfaces seen in reflections", r"rtggx_set_sun_reflections\(ctx, 1\) lifts the limit"))


def test_the_executable_refuses_the_flag_without_a_sun_before_asking_for_a_device(built):
    HS.executable_refuses([["-sunreflections"], ["-recursion", "2", "-sunreflections"], ["-sunreflections", "-spp", "2"]], must_mention="-sunreflections")


def frame(cls, metallic, depth=1, samples=1, sun=(L, E), reflections=None):
    """(RayTracingOut0, RayTracingOut1, rays, the oracle's record) of one frame of `cls` on the golden scene."""
    kw = dict(depth=depth, samples=samples)
    o = cls(W, H, **kw) if cls is not O.Oracle else O.Oracle(W, H)
    try:
        HS.scene(o, metallic=metallic)
        if sun is not None:
            o.set_sun(*sun)
        if reflections is not None:
            o.set_sun_reflections(reflections)
        rays = o.ray_trace()
        rec = dict(counts=o.counts.copy(), lit=o.lit.copy(), hit_rays=o.hit_rays) if cls is SH.Oracle else None
        return o.buffer(O.BUF_RT_REFL), o.buffer(O.BUF_RT_DIFF), rays, rec
    finally:
        o.close()


CASES = [(1, 1), (2, 1), (1, 2), (2, 2)]


@pytest.fixture(scope="module")
def sun_alone():
    """tests/sun_ref.cpp's frames, by (depth, samples)."""
    return {k: frame(SR.Oracle, MIXED, *k) for k in CASES}


@pytest.fixture(scope="module")
def with_hits():
    return {k: frame(SH.Oracle, MIXED, *k, reflections=True) for k in CASES}


@pytest.mark.parametrize("depth,samples", CASES)
def test_with_the_toggle_off_the_frame_is_sun_refs(sun_alone, depth, samples):
    want = sun_alone[(depth, samples)]
    for reflections in (None, False):
        refl, diff, rays, rec = frame(SH.Oracle, MIXED, depth, samples, reflections=reflections)
        assert np.array_equal(refl, want[0]) and np.array_equal(diff, want[1]) and rays == want[2]
        assert rec["hit_rays"] == 0 and not rec["lit"].any()


def test_without_irradiance_the_frame_is_the_stock_oracles():
    want = frame(O.Oracle, MIXED, sun=None)
    refl, diff, rays, rec = frame(SH.Oracle, MIXED, sun=(L, (0.0, 0.0, 0.0)), reflections=True)
    assert np.array_equal(refl, want[0]) and np.array_equal(diff, want[1]) and rays == want[2] and rec["hit_rays"] == 0


@pytest.mark.parametrize("depth,samples", CASES)
def test_words_change_only_where_a_hit_is_lit_and_never_get_darker(sun_alone, with_hits, depth, samples):
    refl, diff, rays, rec = with_hits[(depth, samples)]
    want = sun_alone[(depth, samples)]
    for bit, got, base in ((1, refl, want[0]), (2, diff, want[1])):
        lit = (rec["lit"] & bit) != 0
        assert lit.any() and np.array_equal(got[~lit], base[~lit])
        assert (O.unpack_r11g11b10f(got[lit]) >= O.unpack_r11g11b10f(base[lit])).all()
        assert (got[lit] != base[lit]).any()
    assert rays == want[2] + rec["hit_rays"] and rec["hit_rays"] > 0


def test_all_metal_leaves_the_carry_over_alone():
    _, diff0, _, _ = frame(SR.Oracle, (1.0, 1.0), 2)
    refl, diff, _, rec = frame(SH.Oracle, (1.0, 1.0), 2, reflections=True)
    assert np.array_equal(diff, diff0) and (rec["lit"] & 1).any() and not (rec["lit"] & 2).any()


def test_the_class_shares_of_the_scene_the_gpu_tests_use(with_hits):
    """The golden file's conditions, met by the restatement alone: among level-0 touched hits every class holds a twentieth; at depth 2
    every class has 20 level-1 hits; both lobes occur; and metallic (0.0, 1.0) has preset returns."""
    counts = with_hits[(2, 1)][3]["counts"]
    got = {"level%d" % d: {k: int(counts[d][SH.COLUMNS.index(k)]) for k in SH.COLUMNS} for d in range(2)}
    assert got == {k: GOLDEN[k] for k in got}, got
    level0 = [got["level0"][k] for k in SH.CLASSES]
    assert min(level0) >= 0.05 * sum(level0), level0
    assert min(got["level1"][k] for k in SH.CLASSES) >= 20, got["level1"]
    assert min(got["level%d" % d][k] for d in range(2) for k in ("specular", "diffuse")) > 0, got
    assert np.array_equal(with_hits[(1, 1)][3]["counts"][0], counts[0])      # (level 0 does not depend on the depth)
    _, _, _, rec = frame(SH.Oracle, tuple(GOLDEN["preset_metallic"]), 2, reflections=True)
    presets = int(rec["counts"][:, SH.COLUMNS.index("preset")].sum())
    assert presets == GOLDEN["preset_returns"] and presets > 0 and rec["hit_rays"] > 0
