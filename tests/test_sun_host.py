"""The sun, the part that needs no GPU: rtggx_set_sun declared, exported and bound; the -sun flag refused at parse time; the restatement
(tests/sun_ref.cpp) against the stock oracle; and the class shares of the scene and direction the GPU tests use (tests/golden/sun_classes.json)."""
import json
import os

import numpy as np
import pytest

import host_support as HS
import sun_ref as SR
from oracle import oracle as O

GOLDEN = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "sun_classes.json")))
L, E = GOLDEN["direction"], GOLDEN["irradiance"]
W, H = GOLDEN["width"], GOLDEN["height"]


def test_the_entry_point_is_declared_exported_and_bound(built):
    HS.declared_exported_bound(
        "rtggx_set_sun", r"\bint\s+rtggx_set_sun\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*const\s+float\s+direction\s*\[3\]\s*,\s*const\s+float\s+irradiance\s*\[3\]\s*\)",
        defines=(r"\bRTGGX_BUF_COUNT\s*=\s*28\b", r"Known limit: surfaces seen in reflections"))
    from raytracedggx_amd import capi
    assert "rtggx_trace_occlusion" in capi.EXPORTS and callable(capi.Context.trace_occlusion)


def test_the_executable_refuses_a_bad_sun_before_asking_for_a_device(built):
    HS.executable_refuses([["-sun", "1", "2", "3"], ["-sun", "0", "0", "0", "1", "1", "1"], ["-sun", "0", "1", "0", "1", "-1", "1"],
                           ["-sun", "0", "1", "0", "1", "1", "1", "-rayrate", "4"], ["-rayrate", "4", "-sun", "0", "1", "0", "1", "1", "1"]], must_mention="-sun")


def test_host_normalisation_is_double_rounded_once():
    for d in ((0.35, 0.8, -0.5), (3e-20, 4e-20, 0.0), (1e19, 1e19, 1e19), (0.0, -7.0, 0.0)):
        n = SR.normalise(d)
        x = np.asarray(d, np.float32).astype(np.float64)
        assert n.dtype == np.float32 and np.array_equal(n, (x / np.linalg.norm(x)).astype(np.float32))
        assert abs(float(np.linalg.norm(n.astype(np.float64))) - 1.0) < 2e-7      # (a fp32 computation of the length would overflow or flush on two of these)


def frames(metallic, sun):
    """(RayTracingOut0, RayTracingOut1, rays, class map) of the restatement's frame on the 100 x 54 bunny."""
    o = SR.Oracle(W, H, entry="depth")
    try:
        HS.scene(o, metallic=metallic)
        if sun is not None:
            o.set_sun(*sun)
        rays = o.ray_trace()
        return o.buffer(O.BUF_RT_REFL), o.buffer(O.BUF_RT_DIFF), rays, o.classes.copy()
    finally:
        o.close()


@pytest.fixture(scope="module")
def stock():
    """The stock oracle's frame, mixed materials."""
    o = O.Oracle(W, H)
    try:
        HS.scene(o, metallic=tuple(GOLDEN["metallic"]))
        rays = o.ray_trace()
        return o.buffer(O.BUF_RT_REFL), o.buffer(O.BUF_RT_DIFF), rays
    finally:
        o.close()


@pytest.fixture(scope="module")
def sunlit():
    return frames(tuple(GOLDEN["metallic"]), (L, E))


def test_without_irradiance_the_frame_is_the_stock_oracles(stock):
    refl, diff, rays, _ = frames(tuple(GOLDEN["metallic"]), (L, (0.0, 0.0, 0.0)))
    assert np.array_equal(refl, stock[0]) and np.array_equal(diff, stock[1]) and rays == stock[2]


def test_only_lit_pixels_change_and_never_get_darker(stock, sunlit):
    refl, diff, rays, classes = sunlit
    lit = classes == SR.LIT
    for got, want in ((refl, stock[0]), (diff, stock[1])):
        assert np.array_equal(got[~lit], want[~lit])
        assert (O.unpack_r11g11b10f(got[lit]) >= O.unpack_r11g11b10f(want[lit])).all()
    assert (refl[lit] != stock[0][lit]).any() and (diff[lit] != stock[1][lit]).any()
    assert rays == stock[2] + int((classes >= SR.OCCLUDED).sum())


def test_all_metal_leaves_the_carry_over_alone():
    _, diff0, _, _ = frames((1.0, 1.0), None)
    refl, diff, _, classes = frames((1.0, 1.0), (L, E))
    assert np.array_equal(diff, diff0) and (classes == SR.LIT).any()


def test_every_covered_class_holds_a_twentieth_of_the_covered_pixels(sunlit):
    classes = sunlit[3]
    counts = {"covered": int((classes > 0).sum()), "facing_away": int((classes == SR.FACING_AWAY).sum()),
              "occluded": int((classes == SR.OCCLUDED).sum()), "lit": int((classes == SR.LIT).sum())}
    assert counts == {k: GOLDEN[k] for k in counts}, counts
    for k in ("facing_away", "occluded", "lit"):
        assert counts[k] >= 0.05 * counts["covered"], (k, counts)
