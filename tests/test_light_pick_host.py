"""One shadow ray per surface point for all local lights, the part that needs no GPU: rtggx_set_light_sampling declared, exported and bound,
and the header's rule; -lightpick checked at parse time; the restatement (tests/light_pick_ref.cpp) against tests/light_hit_ref.cpp's frames
in mode 0 and with one casting light; the luminance identity; the draw walked through all its 2^24 values; the hash inputs worked out apart
from it; convergence to mode 0; and the class conditions of the scene the GPU tests use (tests/golden/light_pick_classes.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import host_support as HS
import light_hit_ref as LH
import light_pick_ref as LP
import lights_ref as LR
from oracle import oracle as O

GOLDEN = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "light_pick_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]
FRAMES = GOLDEN["frames"]
SUN = ([-0.6, 0.5, -0.3], [3.0, 3.0, 3.0])
SMALL = (100, 56)      # the frames that are only compared with each other


def test_the_entry_point_is_declared_exported_and_bound(built):
    HS.declared_exported_bound(
        "rtggx_set_light_sampling", r"\bint\s+rtggx_set_light_sampling\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*int\s+mode\s*\)",
        defines=(r"\bRTGGX_BUF_COUNT\s*=\s*28\b", r"#define\s+RTGGX_MAX_LIGHTS\s+8u",
                 r"mode 0 \(default\): every light traces its own shadow ray", r"mode 1: one shadow ray per surface point for all lights",
                 r"Y\(c\) = \(0\.25 c\.r \+ 0\.5 c\.g\) \+ 0\.25 c\.b", r"w_i = Y\(spec_i\) \+ Y\(diff_i\); where m >= 1 w_i = Y\(spec_i\) alone",
                 r"iff w_i > 0 \(a NaN is not a candidate\)", r"W = \(\(\+0 \+ w_a\) \+ w_b\) \+ \.\.\.", r"v = rng\(h \+ 96 \* 0x9E3779B9\)",
                 r"x = \(float\)\(v >> 8\) / 16777216", r"the chosen light is the first with t < c; if none qualifies, the last\s+\*?\s*candidate",
                 r"f = W / w_i, correctly rounded", r"with its own slot 16 \+ i", r"S0_c = spec_i,c f, one more multiplication",
                 r"v = rng\(h \+ \(104 \+ 2 d \+ img\) \*\s+\*?\s*0x9E3779B9\)", r"the slots 104 \.\. 111", r"32 \+ 16 d \+ 8 img \+ i; the term added is s_i f",
                 r"16 bytes per ray slot", r"the pick ignores visibility"),
        method="set_light_sampling")
    from raytracedggx_amd import app, capi
    assert capi.load().rtggx_set_light_sampling.argtypes == [C.c_void_p, C.c_int]
    assert "rtggx_app_set_light_sampling" in app.HOST_EXPORTS and hasattr(C.CDLL(app.HOST_LIB_PATH), "rtggx_app_set_light_sampling")
    assert callable(getattr(app.RayTracedGGX, "set_light_sampling", None))
    for name in ("RayTracedGGX.h", "RayTracedGGX.cpp"):      # the flag list and kFlags
        text = open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", name)).read()
        assert "-lightpick" in text or '"lightpick"' in text
    assert "SetLightSampling" in open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", "RayTracer.h")).read()


POINT = ["-light", "1", "2", "3", "4", "5", "6", "7"]
SPOT = ["-spot", "1", "2", "3", "4", "5", "6", "9", "0.5", "0", "-1", "0", "30", "20"]


def test_the_executable_refuses_the_flag_without_lights_before_asking_for_a_device(built):
    HS.executable_refuses([
        (["-lightpick"], "-lightpick"), (["-lightpick", "-rayrate", "4"], "-lightpick"),
        (["-sun", "0", "1", "0", "1", "1", "1", "-sunreflections", "-lightpick"], "-lightpick"),
        (["-lightpick"] + POINT + ["-rayrate", "4"], "-rayrate 4"), (SPOT + ["-rayrate", "4", "-lightpick"], "-rayrate 4"),
        (["-lightpick", "-lightreflections"], "-light")])


def test_the_executable_parses_the_flag_with_lights(built, tmp_path):
    """What stops these runs is the environment file, which is read after the command line and before a device is asked for."""
    import assets
    missing = str(tmp_path / "missing.hdr")
    HS.executable_refuses([["-env", missing, "-lightpick"] + POINT, ["-env", missing] + SPOT + ["-lightpick"],
                           ["-env", missing] + POINT + ["-lightpick", "-lightreflections"] + SPOT + ["-sun", "0", "1", "0", "1", "1", "1", "-sunreflections", "-recursion", "2"]],
                          must_mention="cannot open", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def frame(cls, size, lights=LIGHTS, sun=False, depth=1, samples=1, metallic=MIXED, reflections=1, mode=None, force_walker=False):
    o = cls(size[0], size[1], depth=depth, samples=samples)
    try:
        HS.scene(o, metallic=metallic)
        if sun:
            o.set_sun(*SUN); o.set_sun_reflections(True); o.set_sun_angle(5.0)
        o.set_lights(lights)
        o.set_light_reflections(reflections)
        if mode is not None:
            o.set_light_sampling(mode)
            o.force_walker = force_walker
        rays = o.ray_trace()
        return dict(refl=o.buffer(O.BUF_RT_REFL), diff=o.buffer(O.BUF_RT_DIFF), rays=rays, classes=o.classes.copy(), light_classes=o.light_classes.copy(),
                    hit_rays=o.light_hit_rays, light_lit=o.light_lit.copy(), counts=o.light_counts.copy())
    finally:
        o.close()


@pytest.mark.parametrize("sun,depth,samples", [(False, 1, 1), (True, 2, 1), (False, 2, 2)], ids=["D = 1", "the sun, D = 2", "D = 2, N = 2"])
def test_mode_0_is_light_hit_refs_frame(sun, depth, samples):
    """The copied walker has not drifted: in mode 0 (the walker forced) the frame, the classes, the counts and the ray count are
    light_hit_ref's -- and so are those of a mode-1 oracle whose lights cast no ray or that has none."""
    kw = dict(sun=sun, depth=depth, samples=samples)
    want = frame(LH.Oracle, SMALL, **kw)
    got = frame(LP.Oracle, SMALL, mode=0, force_walker=True, **kw)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert want["hit_rays"] > 0
    dark = [dict(l, intensity=[0.0, 0.0, 0.0]) for l in LIGHTS]
    for lights in (dark, []):
        want = frame(LH.Oracle, SMALL, lights=lights, **kw)
        got = frame(LP.Oracle, SMALL, lights=lights, mode=1, **kw)
        for k in want:
            assert np.array_equal(got[k], want[k]), (len(lights), k)


@pytest.mark.parametrize("radius", [0.0, 0.5], ids=["radius 0", "radius 0.5"])
def test_one_casting_light_is_mode_0_bit_for_bit(radius):
    """Every pick is that light and f is exactly 1: both images and the ray count are mode 0's, at the primary surface and at the hits of
    a depth-2 frame.  A light without an intensity in front keeps its index, and the casting light its slots."""
    lights = [dict(LIGHTS[0], intensity=[0.0, 0.0, 0.0]), dict(LIGHTS[2], radius=radius)]
    want = frame(LH.Oracle, (W, H), lights=lights, depth=2)
    got = frame(LP.Oracle, (W, H), lights=lights, depth=2, mode=1)
    assert np.array_equal(got["refl"], want["refl"]) and np.array_equal(got["diff"], want["diff"]) and got["rays"] == want["rays"]
    assert got["hit_rays"] == want["hit_rays"] > 0 and (want["light_classes"] == LR.LIT).any() and (want["light_classes"] == LR.OCCLUDED).any()


def test_the_restatement_refuses_other_modes():
    o = LP.Oracle(16, 16)
    try:
        o.set_light_sampling(1)
        for bad in (2, -1, 256, True):
            with pytest.raises(ValueError):
                o.set_light_sampling(bad)
        assert o.light_sampling == 1
    finally:
        o.close()


# ---- the estimator ----------------------------------------------------------------------------------------------------------------------
def picking_oracle(lights=LIGHTS, unoccluded=False, metallic=MIXED):
    """A mode-1 oracle of the golden scene, one frame traced; (oracle, base frame index)."""
    o = LP.Oracle(W, H)
    HS.scene(o, metallic=metallic)
    o.set_lights(lights); o.set_light_sampling(1)
    o.unoccluded = unoccluded
    base = HS.frame_index(o)
    o.ray_trace()
    return o, base


# Y(S0) + Y(S1), summed in float64 from the fp32 terms, against the fp32 W.  With u = 2^-24, every quantity positive: w_i is the exact
# Y(spec_i) + Y(diff_i) times (1 + e), |e| <= 3u (the multiplications by 0.25 and 0.5 are exact; two roundings inside either Y -- they act
# on parts of the sum, so together no more than 2u of the whole -- and one for the sum of the two); f = W / w_i adds u; every component of
# S = spec f or diff f adds u, and a weighted sum of components each off by at most u is off by at most u.  First order 5u; 6u covers the
# products of the errors.  (A wrong pick -- another light's terms under the chosen light's f -- or a wrong f misses by the ratio of two
# lights' weights.)
LUMINANCE_BOUND = 6.0 * 2.0 ** -24
assert LUMINANCE_BOUND < 1e-4


def test_the_luminance_of_the_term_is_W():
    o, _ = picking_oracle(unoccluded=True)
    try:
        info, wf, terms = o.pick_info.astype(int), o.pick_wf.astype(np.float64), o.pick_terms
        ray = np.isin(info[..., 2], (LR.OCCLUDED, LR.LIT))
        assert ray.sum() > 2000 and not (info[..., 2] == LR.OCCLUDED).any() and (info[ray, 0] >= 2).sum() > 1000
        y = LP.luminance(terms[..., :3]) + LP.luminance(terms[..., 3:])
        rel = np.abs(y[ray] - wf[ray, 0]) / wf[ray, 0]
        print("luminance identity: %d rays, largest relative difference %.3e (bound %.3e)" % (ray.sum(), rel.max(), LUMINANCE_BOUND))
        assert rel.max() <= LUMINANCE_BOUND, rel.max()
        single = ray & (info[..., 0] == 1)
        assert single.any() and (wf[single, 1] == 1.0).all()      # a single candidate: f is exactly 1
        assert (wf[ray & (info[..., 0] >= 2), 1] > 1.0).all()
    finally:
        o.close()


def test_the_values_of_the_draw_that_choose_a_light_form_one_interval_of_its_share():
    """At 8 pixels with two candidates or more, three among them where there are that many: all 2^24 values of v >> 8."""
    o, _ = picking_oracle()
    try:
        n = o.pick_info[..., 0].astype(int)
        weights, Wsum = o.pick_weights.reshape(-1, 8), o.pick_wf[..., 0].reshape(-1)
        three, two = np.flatnonzero(n.reshape(-1) >= 3), np.flatnonzero(n.reshape(-1) == 2)
        assert len(three) >= 3 and len(two) >= 5
        chosen = [int(three[(len(three) * k) // 3]) for k in range(3)] + [int(two[(len(two) * k) // 5]) for k in range(5)]
        assert len(set(chosen)) == 8
        for pix in chosen:
            w = weights[pix]
            got = LP.intervals(w)
            assert sum(c for c, _, _ in got) == 1 << 24, pix
            at = 0
            for i, (count, first, last) in enumerate(got):
                if not w[i] > 0:
                    assert count == 0, (pix, i)
                    continue
                assert count > 0 and first == at and last - first + 1 == count, (pix, i, got)      # contiguous, in the order of the lights
                at = last + 1
                share = float(w[i]) / float(Wsum[pix])
                assert abs(count / float(1 << 24) - share) <= 2.0 ** -22, (pix, i, count, share)
    finally:
        o.close()


def test_the_hash_inputs_worked_out_by_hand():
    """(pixel, frame index, slot) -> v from Python integers against the restatement's; the nine slots meet no other feature's."""
    slots = {LP.PICK_SLOT} | {LP.hit_slot(d, img) for d in range(4) for img in range(2)}
    assert len(slots) == 9 and slots == {96} | set(range(104, 112))
    assert not slots & (set(range(0, 9)) | set(range(16, 24)) | {LH.slot(d, img, i) for d in range(4) for img in range(2) for i in range(8)})
    seen = set()
    for case in ((0, 0, 96), (1, 0, 96), (12431, 1, 104), (12431, 1, 105), (2073599, 4000000000, 111), (77, 12345, 106)):
        want = LP.draw_word(*case)
        assert want == LP.draw_word_lib(*case), case
        seen.add(want)
    assert len(seen) == 6
    # the draw's word is not the word a light's target is drawn from
    assert LP.draw_word(7, 3, 96) not in {LH.sample_words(7, 3, d, img, i)[0] for d in range(4) for img in range(2) for i in range(8)}


def convergence():
    """The three golden lights at radius 0, where mode 0 is deterministic: the relative L2 error, over the pixels that have a term, of the
    mean of the mode-1 fp32 terms over frames 0 .. 63 and over frames 0 .. 255 against mode 0's S."""
    lights = [dict(l, radius=0.0) for l in LIGHTS]
    # mode 0's S in fp32: with radius 0 a light alone in mode 1 is that light's term of mode 0 (f = 1, no hash), added in index order
    S = np.zeros((H, W, 6), np.float32)
    for i in range(len(lights)):
        alone = [dict(l, intensity=l["intensity"] if k == i else [0.0, 0.0, 0.0]) for k, l in enumerate(lights)]
        o, _ = picking_oracle(alone)
        S = S + o.pick_terms
        o.close()
    o, base = picking_oracle(lights)
    try:
        has = S.any(-1)
        total, err = np.zeros((H, W, 6), np.float64), {}
        for f in range(256):
            HS.set_frame_index(o, base + f)
            o.lights_apply()
            total += o.pick_terms
            if f + 1 in (64, 256):
                mean = total / (f + 1)
                err[f + 1] = float(np.sqrt(((mean - S)[has] ** 2).sum() / (S[has].astype(np.float64) ** 2).sum()))
        return err[64], err[256], int(has.sum())
    finally:
        o.close()


def test_the_mean_over_frames_converges_to_mode_0():
    """An unbiased estimator halves its error from 64 to 256 frames; a biased one plateaus.  The margin to 0.7 is for finite-sample noise."""
    e64, e256, pixels = convergence()
    print("convergence: %d pixels, relative L2 %.5f after 64 frames, %.5f after 256" % (pixels, e64, e256))
    assert pixels > 2000
    assert e256 < 0.7 * e64, (e64, e256)
    assert abs(e64 - GOLDEN["convergence"]["frames64"]) <= 1e-9 and abs(e256 - GOLDEN["convergence"]["frames256"]) <= 1e-9, (e64, e256)


# ---- the class conditions of the scene the GPU tests use ---------------------------------------------------------------------------------
def golden_figures(depth):
    o = LP.Oracle(W, H, depth=depth)
    try:
        HS.scene(o, metallic=MIXED)
        base = HS.frame_index(o)
        o.set_lights(LIGHTS); o.set_light_reflections(1 if depth >= 2 else 0); o.set_light_sampling(1)
        frames = []
        for f in range(FRAMES):
            HS.set_frame_index(o, base + f)
            o.ray_trace()
            frames.append(LP.record(o))
        return LP.figures(frames, len(LIGHTS), depth >= 2)
    finally:
        o.close()


@pytest.mark.parametrize("depth", [1, 2], ids=["depth 1", "depth 2, the lights at the hits"])
def test_the_class_conditions_of_the_scene_the_gpu_tests_use(depth):
    """lights_classes.json's scene and lights A, B and C over the first FRAMES frame indices of the still scene: the conditions hold on the
    restatement alone -- of the primary pass, and at depth 2 of the hits --, and the counts are the golden file's."""
    assert {k: GOLDEN[k] for k in ("width", "height", "metallic", "lights", "spot_degrees", "frames")} == {
        k: json.load(open(os.path.join(HS.ROOT, "tests", "golden", "lights_classes.json")))[k] for k in ("width", "height", "metallic", "lights", "spot_degrees", "frames")}
    assert GOLDEN["columns"] == list(LP.COLUMNS)
    got = golden_figures(depth)
    assert got == GOLDEN["depth%d" % depth], got
    assert ("hits" in got) == (depth >= 2)
    LP.check_conditions(got, "golden, depth %d" % depth)
