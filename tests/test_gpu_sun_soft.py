"""A sun with a size, on the GPU (rtggx_set_sun_angle; lighting.hip sunGenKernel<true>, sunHitGenKernel<true>): frames bit for bit against
the restatement (tests/sun_soft_ref.cpp) at depth 1 and 2, with several samples, a sample map, the other sampler and a larger sample set; a
small disk; all-metal materials; twins; refusals; accumulation and the penumbra in its mean; strips; a deforming mesh; still sky; a 1080p
frame.  Scene, direction, irradiance and angle are those of tests/golden/sun_soft_classes.json, whose class conditions
tests/test_sun_soft_host.py establishes on the CPU over 8 frames: 100 pixels that are lit in one frame and occluded in another, 20 with a
sample below the horizon, 20 hits of either kind.  The tests that compare frames with the restatement run 8 frames of their own and
assert the same bars on them."""
import json
import os

import numpy as np
import pytest

import accum_ref as AR
import adaptive_ref as AD
import gpu_support as G
import sun_soft_ref as SS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sun_soft_classes.json")))
L, E = GOLDEN["direction"], GOLDEN["irradiance"]
W, H = GOLDEN["width"], GOLDEN["height"]      # 148 x 84: ragged right and bottom edges (no multiple of 8 or 16), 10 x 6 tiles
MIXED = tuple(GOLDEN["metallic"])
ANGLE = GOLDEN["angle"]
SUN_ARGS = ["-sun"] + [str(x) for x in L + E]
METAL_ARGS = ["-metallic", str(MIXED[0]), str(MIXED[1])]
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
BAR_MIXED, BAR_BELOW, BAR_HITS = 100, 20, 20      # the golden file's conditions, over its 8 frames
FRAMES = GOLDEN["frames"]


def soft_pair(width, height, metallic=MIXED, depth=1, samples=1, sample_set=256, vndf=False, reflections=False, angle=ANGLE):
    """gpu_support.restated_pair with this feature's oracle, both sides lit and with the angle."""
    p = G.Pair(width, height, metallic=metallic, oracle=lambda w, h: SS.Oracle(w, h, depth=depth, samples=samples, sample_set=sample_set))
    p.ctx.set_sample_set(sample_set)
    if samples != 1:
        p.ctx.set_samples_per_pixel(samples)
    if depth != 1:
        p.ctx.set_max_recursion_depth(depth)
    if vndf:
        p.ctx.set_sampler(True); p.o.set_sampler(True)
    p.ctx.set_sun(L, E); p.o.set_sun(L, E)
    if reflections:
        p.ctx.set_sun_reflections(1); p.o.set_sun_reflections(True)
    p.ctx.set_sun_angle(angle); p.o.set_sun_angle(angle)
    p.o.statistics = True
    return p


class Conditions:
    """The class conditions over a test's frames: take() after every frame the oracle has traced (a mapped frame: its parts composed)."""

    def __init__(self):
        self.classes, self.differs = [], None
        self.hits_below = self.hits_differ = 0

    def take(self, o):
        self.classes.append(o.classes.copy())
        d = o.classes != o.centre
        self.differs = d if self.differs is None else self.differs | d
        self.hits_below += o.soft_count("below_horizon"); self.hits_differ += o.soft_count("differs")

    def figures(self, label):
        c = np.stack(self.classes)
        got = dict(mixed=int(((c == SS.LIT).any(0) & (c == SS.OCCLUDED).any(0)).sum()), below=int((c == SS.BELOW_HORIZON).any(0).sum()),
                   differs=int(self.differs.sum()), hits_below=self.hits_below, hits_differ=self.hits_differ)
        print("%s, %d frames: %s" % (label, len(self.classes), got))
        return got

    def check(self, label, reflections):
        """100 pixels lit in one frame and occluded in another, 20 with a sample below the horizon; with the toggle 20 hits of each kind."""
        got = self.figures(label)
        assert got["mixed"] >= BAR_MIXED and got["below"] >= BAR_BELOW, (label, got)
        assert not reflections or (got["hits_below"] >= BAR_HITS and got["hits_differ"] >= BAR_HITS), (label, got)


SETTINGS = [dict(), dict(depth=2, reflections=True), dict(samples=2, reflections=True), dict(samples=4, reflections=True, mapped=True),
            dict(vndf=True, depth=2, reflections=True), dict(sample_set=1024, depth=2, reflections=True)]
IDS = ["depth 1", "depth 2 with reflections", "N = 2 with reflections", "N = 4 mapped 1 2 4", "VNDF", "M = 1024"]


def mapped_or_plain_frame(p, blocks):
    if blocks is None:
        p.frame()
        return
    p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
    p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
    p.o.update_as(); p.o.render_visibility()
    p.rays = SS.mapped_frame(p.o, blocks)
    p.o.denoise(); p.o.tone_map()


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_frames_equal_the_restatement(built, setting):
    """148 x 84 bunny, metallic (0.25, 0.75), 5 degrees.  Three frames: G-buffer, RayTracingOut0/1 and the ray count bit for bit / equal, the
    denoised images under the existing bars.  The class conditions are defined over 8 frames, so five more follow, their raw words and ray
    counts compared as well, and the conditions are asserted on the eight at the golden file's bars.  M = 1024: the restatement draws the
    disk with the 256-entry table whatever the sample set is.  Under the map the classes of a frame are those of its parts, composed."""
    setting = dict(setting)
    mapped = setting.pop("mapped", False)
    p = soft_pair(W, H, **setting)
    cond = Conditions()
    try:
        blocks = None
        if mapped:
            by, bx = AD.blocks_of(W, H)
            y, x = np.mgrid[0:by, 0:bx]
            blocks = np.array([1, 2, 4], np.uint8)[(x + 2 * y) % 3]
            p.ctx.set_sample_map(blocks)
        for f in range(FRAMES):
            label = "frame %d" % f
            mapped_or_plain_frame(p, blocks)
            G.check_raw(p, label, require_rays=True)
            if f < 3:
                p.check_frame(label)
            cond.take(p.o)
        cond.check(str(setting) + (" mapped" if mapped else ""), setting.get("reflections", False))
    finally:
        p.close()


def test_a_small_disk_equals_the_restatement(built):
    """The same three frames at 0.25 degrees, depth 2 with the toggle: k = 9.5e-6, where sin(theta) needs e (2 - e).  The class conditions
    are those of 5 degrees and a disk a twentieth as wide CANNOT meet them -- its penumbrae hold a twentieth of the 228 mixed pixels -- so
    none of the bars is asserted here; what is asserted is that the disk does something at all in these frames: at least one pixel whose
    sampled ray ends otherwise than the centre ray, and at least one pixel below the horizon."""
    p = soft_pair(W, H, depth=2, reflections=True, angle=0.25)
    cond = Conditions()
    try:
        for f in range(3):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            p.check_frame("frame %d" % f)
            cond.take(p.o)
        got = cond.figures("0.25 degrees")
        assert got["differs"] >= 1 and got["below"] >= 1, got
    finally:
        p.close()


def test_all_metal_leaves_the_carry_over_alone(built):
    """Default materials: no diffuse path -- RayTracingOut1 equals the restatement's and a sunless twin's."""
    p, b = soft_pair(W, H, metallic=None, depth=2, reflections=True), G.app(W, H, ["-recursion", "2"])
    try:
        for f in range(3):
            p.frame(); G.frame(b)
            G.check_raw(p, "frame %d" % f, require_rays=True)
            ib = G.images(b, ("diff", "refl"))
            np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), ib["diff"], err_msg="frame %d: RayTracingOut1" % f)
            assert (p.ctx.readback(p.capi.BUF_RT_REFL) != ib["refl"]).any()
    finally:
        p.close(); b.OnDestroy()


def twins(a, b, frames, label, denoised=True):
    for f in range(frames):
        G.frame(a); G.frame(b)
        names = IMAGES if denoised else G.GBUFFER + G.RAW + G.RAYS
        G.assert_same(G.images(a, names), G.images(b, names), "%s, frame %d" % (label, f))
        assert a.context.placement() == b.context.placement(), "%s, frame %d: placement" % (label, f)


def test_an_angle_without_a_sun_is_a_default_context(built):
    a, b = G.app(320, 180, METAL_ARGS), G.app(320, 180, METAL_ARGS)
    try:
        a.context.set_sun_angle(ANGLE); a.context.set_sun_reflections(1)
        twins(a, b, 3, "an angle, no sun")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_an_angle_set_back_to_0_before_the_next_frame_is_the_directional_sun(built):
    extra = METAL_ARGS + SUN_ARGS + ["-sunreflections", "-recursion", "2"]
    a, b = G.app(320, 180, extra), G.app(320, 180, extra)
    try:
        twins(a, b, 1, "before")
        a.context.set_sun_angle(ANGLE); a.context.set_sun_angle(0.0)
        twins(a, b, 3, "an angle set and taken back")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_angle_0_from_the_start_is_the_directional_sun(built):
    extra = METAL_ARGS + SUN_ARGS + ["-sunreflections", "-recursion", "2"]
    a, b = G.app(320, 180, extra + ["-sunangle", "0"]), G.app(320, 180, extra)
    try:
        a.context.set_sun_angle(0.0)
        twins(a, b, 3, "angle 0")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_the_flag_is_the_call(built):
    extra = METAL_ARGS + SUN_ARGS + ["-sunreflections", "-recursion", "2"]
    a, b = G.app(W, H, extra + ["-sunangle", str(ANGLE)]), G.app(W, H, extra)
    try:
        b.context.set_sun_angle(ANGLE)
        twins(a, b, 2, "-sunangle")
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_refused_values_leave_the_setting_as_it_was(built):
    from raytracedggx_amd import capi
    p = soft_pair(W, H, depth=2, reflections=True)
    try:
        p.frame(); G.check_raw(p, "before", require_rays=True)
        for bad in (float("nan"), -1.0, -1e-30, 10.5, float("inf"), float("-inf")):
            with pytest.raises(capi.RtggxError, match="rtggx_set_sun_angle"):
                p.ctx.set_sun_angle(bad)
            with pytest.raises(ValueError):
                p.o.set_sun_angle(bad)
        p.frame(); G.check_raw(p, "refused at %g degrees" % ANGLE, require_rays=True)
        assert (p.o.classes != p.o.centre).any()
        p.ctx.set_sun_angle(0.0); p.o.set_sun_angle(0.0)
        with pytest.raises(capi.RtggxError, match="rtggx_set_sun_angle"):
            p.ctx.set_sun_angle(11.0)
        p.frame(); G.check_raw(p, "refused at 0 degrees", require_rays=True)
        p.ctx.set_sun_angle(10.0); p.o.set_sun_angle(10.0)      # the cap itself is allowed
        p.frame(); G.check_raw(p, "10 degrees", require_rays=True)
    finally:
        p.close()


def test_accumulated_sums_and_the_penumbra_in_their_mean(built):
    """8 accumulated frames at depth 1: the sums bit for bit against accum_ref over the restatement's frames; and the penumbra itself -- at
    least 100 pixels whose accumulated RayTracingOut0 lies strictly between the sums of the sunless words and of the directional sun's lit
    words of the same frames, some of them pixels where the directional sun's shadow does not move at all in those frames."""
    from raytracedggx_amd import capi
    p = soft_pair(W, H)
    try:
        c = p.ctx
        c.set_accumulation(True)
        acc, none, lit = AR.Accumulator(H, W), AR.Accumulator(H, W), AR.Accumulator(H, W)
        centre = []
        for f in range(8):
            p.frame()
            G.check_raw(p, "frame %d" % f, require_rays=True)
            vis = p.o.buffer(O.BUF_VISIBILITY)
            acc.add(p.o.buffer(O.BUF_RT_REFL), p.o.buffer(O.BUF_RT_DIFF), vis, MIXED)
            assert c.accumulated_frames() == acc.frames
            for got, want in ((c.readback(capi.BUF_ACC_REFL), acc.refl), (c.readback(capi.BUF_ACC_DIFF), acc.diff)):
                assert AR.same_bits(got, want).all(), "frame %d" % f
            centre.append(p.o.centre.copy())
            # the same frame without a sun, and with the directional sun unoccluded (both metallics are below 1: no word is a carry-over);
            # the oracle's raw words are put back
            words = p.o.buffer(O.BUF_RT_REFL), p.o.buffer(O.BUF_RT_DIFF)
            sun, p.o.sun = p.o.sun, None
            p.o.ray_trace()
            p.o.sun = sun
            none.add(p.o.buffer(O.BUF_RT_REFL), p.o.buffer(O.BUF_RT_DIFF), vis, MIXED)
            lw = p.o.lit_words()
            lit.add(lw[0], lw[1], vis, MIXED)
            p.o.buffer(O.BUF_RT_REFL, copy=False)[...], p.o.buffer(O.BUF_RT_DIFF, copy=False)[...] = words
        got = c.readback(capi.BUF_ACC_REFL)[..., :3].astype(np.float64).sum(-1)
        lo, hi = none.refl[..., :3].astype(np.float64).sum(-1), lit.refl[..., :3].astype(np.float64).sum(-1)
        between = (got > lo) & (got < hi)
        still = (np.stack(centre) == centre[0]).all(0)
        print("pixels strictly between: %d, of them under a directional shadow edge that does not move: %d" % (int(between.sum()), int((between & still).sum())))
        assert between.sum() >= 100 and (between & still).any()
    finally:
        p.close()


def test_strips_equal_the_full_frame(built):
    extra = tuple(SUN_ARGS) + ("-sunreflections", "-recursion", "2", "-sunangle", str(ANGLE)) + tuple(METAL_ARGS)
    assert G.strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=extra) > 0


def test_a_deforming_mesh_moves_the_penumbra(built):
    """gpu_support.wave, three frames at depth 2: each frame equals the restatement on the moved mesh and the refitted tree."""
    import assets
    p = soft_pair(320, 180, depth=2, reflections=True)
    try:
        p.frame(); G.check_raw(p, "before the deformation", require_rays=True)
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
            assert (p.o.classes != p.o.centre).any() and (p.o.classes == SS.BELOW_HORIZON).any()
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()


def test_still_sky_runs_go_on_across_the_call(built):
    """A still camera and a sun: the runs of the tiles nothing is drawn in keep growing across the call, and the images equal those of a
    context that leaves no tile alone."""
    a, b = G.app(320, 180, SUN_ARGS), G.app(320, 180, SUN_ARGS)
    try:
        b.context.static_sky(False)
        before = None
        for f in range(20):
            if f == 14:
                before = a.context.sky_runs()[0].copy()
                a.context.set_sun_angle(ANGLE); b.context.set_sun_angle(ANGLE)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
        runs, threshold = a.context.sky_runs()
        assert (before >= threshold).any() and (runs[before >= threshold] > before[before >= threshold]).all()
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_a_1080p_frame_equals_the_restatement(built):
    """The second of two frames at depth 2 with the toggle on: the resident launch shape, the main stream and its spill part, with the
    new directions."""
    p = soft_pair(1920, 1080, depth=2, reflections=True)
    p.o.statistics = False
    try:
        for f in range(2):
            p.frame()
        G.check_raw(p, "1080p", require_rays=True)
        assert (p.o.classes == SS.BELOW_HORIZON).any() and p.o.soft_count("below_horizon") > 0
        key, where = p.ctx.placement()
        assert not key["small"] and where["shade"] == "main", (key, where)
    finally:
        p.close()
