"""The pick weighted by what the pixel remembers, the part that needs no GPU: rtggx_set_light_pick_visibility and rtggx_read_light_visibility
declared, exported and bound, the record's 16 bytes, -lightvisibility checked at parse time; the restatement (tests/light_vis_ref.cpp) against
tests/light_pick_ref.cpp's frames with the setting off and with one casting light; the update's table; the draw walked through all its 2^24
values on weighted candidates; convergence to mode 0 with the history as it comes and with the history overwritten by arbitrary bytes; that it
helps on a scene where mode 1 wastes rays; and the class conditions of a camera that moves, stands and jumps
(tests/golden/light_vis_classes.json)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import host_support as HS
import light_hit_ref as LH
import light_pick_ref as LP
import light_vis_ref as LV
import lights_ref as LR
from oracle import oracle as O

GOLDEN = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "light_vis_classes.json")))
W, H = GOLDEN["width"], GOLDEN["height"]
MIXED = tuple(GOLDEN["metallic"])
LIGHTS = GOLDEN["lights"]
HARD = [dict(l, radius=0.0) for l in LIGHTS]      # radius 0, where mode 0 is deterministic: the estimator's tests
SMALL = (100, 56)      # the frames that are only compared with each other


def test_the_entry_points_are_declared_exported_and_bound(built, tmp_path):
    HS.declared_exported_bound(
        "rtggx_set_light_pick_visibility", r"\bint\s+rtggx_set_light_pick_visibility\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*int\s+enable\s*\)",
        defines=(r"\bRTGGX_BUF_COUNT\s*=\s*28\b", r"#define\s+RTGGX_LIGHT_VIS_FLOOR\s+16u", r"typedef struct RtggxLightVisRecord",
                 r"uint8_t\s+v\[8\];", r"uint32_t\s+normal;", r"uint32_t\s+stamp;",
                 r"qx = floor\(\(\(float\)x \+ 0\.5f\) - vx \(float\)W\)", r"R\.stamp >> 8 == \(s - 1\) & 0xFFFFFF", r"\(R\.stamp & 0xFF\) == inst \+ 1",
                 r"u_i = w_i \(float\)max\(v_i, RTGGX_LIGHT_VIS_FLOOR\)", r"f = U / u_i", r"unoccluded v' = v \+ \(\(255 - v \+ 3\) >> 2\)",
                 r"occluded v' = v - \(\(v \+ 3\) >> 2\)", r"the hits are not covered", r"1/16 of its share", r"not filtered over neighbours"),
        method="set_light_pick_visibility")
    HS.declared_exported_bound(
        "rtggx_read_light_visibility",
        r"\bint\s+rtggx_read_light_visibility\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*uint32_t\s+image\s*(/\*.*?\*/)?\s*,\s*RtggxLightVisRecord\s*\*\s*out\s*,\s*size_t\s+bytes\s*,\s*uint32_t\s*\*\s*sequence\s*\)",
        method="read_light_visibility")
    from raytracedggx_amd import app, capi
    assert capi.load().rtggx_set_light_pick_visibility.argtypes == [C.c_void_p, C.c_int]
    assert capi.LIGHT_VIS_RECORD.itemsize == 16 == LV.RECORD.itemsize and capi.LIGHT_VIS_FLOOR == 16 == LV.FLOOR
    assert [capi.LIGHT_VIS_RECORD.fields[n][1] for n in ("v", "normal", "stamp")] == [0, 8, 12]
    src = tmp_path / "size.c"      # the header's own struct, through a C compiler
    src.write_text('#include "rtggx.h"\n_Static_assert(sizeof(RtggxLightVisRecord) == 16, "16 bytes");\n_Static_assert(RTGGX_LIGHT_VIS_FLOOR == 16u, "floor");\nint main(void) { return 0; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-fsyntax-only", "-I", os.path.join(HS.ROOT, "include"), str(src)])
    assert "rtggx_app_set_light_pick_visibility" in app.HOST_EXPORTS and hasattr(C.CDLL(app.HOST_LIB_PATH), "rtggx_app_set_light_pick_visibility")
    assert callable(getattr(app.RayTracedGGX, "set_light_pick_visibility", None))
    for name in ("RayTracedGGX.h", "RayTracedGGX.cpp"):      # the flag list and kFlags
        text = open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", name)).read()
        assert "-lightvisibility" in text or '"lightvisibility"' in text
    assert "SetLightPickVisibility" in open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", "RayTracer.h")).read()


POINT = ["-light", "1", "2", "3", "4", "5", "6", "7"]


def test_the_executable_refuses_the_flag_where_it_cannot_act_before_asking_for_a_device(built):
    HS.executable_refuses([
        (["-lightvisibility"], "-lightvisibility"), (["-lightvisibility"] + POINT, "-lightvisibility without -lightpick"),
        (["-lightvisibility", "-lightpick"], "-lightpick"),
        (POINT + ["-lightpick", "-lightvisibility", "-strips", "2"], "-lightvisibility: whole frames only"),
        (POINT + ["-lightpick", "-lightvisibility", "-gpus", "2"], "-lightvisibility: whole frames only")])


def test_the_executable_parses_the_flag_with_the_pick(built, tmp_path):
    """What stops these runs is the environment file, which is read after the command line and before a device is asked for."""
    import assets
    missing = str(tmp_path / "missing.hdr")
    HS.executable_refuses([["-env", missing, "-lightpick", "-lightvisibility"] + POINT, ["-env", missing, "-lightvisibility"] + POINT + ["-lightpick", "-lightreflections", "-recursion", "2"]],
                          must_mention="cannot open", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def frames_of(cls, size, lights, mode, vis=None, depth=1, reflections=0, count=2):
    """`count` frames of the still scene under advancing frame indices: per frame both images, the ray count and the lights' rays."""
    o = cls(size[0], size[1], depth=depth)
    try:
        HS.scene(o, metallic=MIXED)
        o.set_lights(lights); o.set_light_reflections(reflections); o.set_light_sampling(mode)
        if vis is not None:
            o.set_light_pick_visibility(vis)
        base, out = HS.frame_index(o), []
        for f in range(count):
            HS.set_frame_index(o, base + f)
            rays = o.ray_trace()
            out.append(dict(refl=o.buffer(O.BUF_RT_REFL), diff=o.buffer(O.BUF_RT_DIFF), rays=rays, light_rays=o.light_rays, info=o.pick_info.copy(), terms=o.pick_terms.copy()))
        return out, (o.seq if hasattr(o, "seq") else None)
    finally:
        o.close()


@pytest.mark.parametrize("mode", [0, 1], ids=["mode 0", "mode 1"])
def test_with_the_setting_off_the_frames_are_light_pick_refs(mode):
    """Never enabled, and enabled then disabled; and in mode 0 the setting on changes nothing either (it acts in mode 1 alone)."""
    want, _ = frames_of(LP.Oracle, SMALL, LIGHTS, mode, depth=2, reflections=1)
    for vis in (None, 0) + ((1,) if mode == 0 else ()):
        got, seq = frames_of(LV.Oracle, SMALL, LIGHTS, mode, vis=vis, depth=2, reflections=1)
        assert seq == 0
        for f, (g, w) in enumerate(zip(got, want)):
            for k in w:
                assert np.array_equal(g[k], w[k]), (vis, f, k)
    assert want[0]["light_rays"] > 0


@pytest.mark.parametrize("radius", [0.0, 0.5], ids=["radius 0", "radius 0.5"])
def test_one_casting_light_is_mode_0_bit_for_bit(radius):
    """Behind a light without an intensity: every pick is that light, f is exactly 1 whatever its byte holds -- four frames equal mode 0's in
    both images and in the ray counts, while the byte moves."""
    lights = [dict(LIGHTS[1], intensity=[0.0, 0.0, 0.0]), dict(LIGHTS[0], radius=radius)]
    want, _ = frames_of(LP.Oracle, (W, H), lights, 0, count=4)
    o = LV.Oracle(W, H)
    try:
        HS.scene(o, metallic=MIXED)
        o.set_lights(lights); o.set_light_sampling(1); o.set_light_pick_visibility(1)
        base = HS.frame_index(o)
        for f in range(4):
            HS.set_frame_index(o, base + f)
            rays = o.ray_trace()
            assert np.array_equal(o.buffer(O.BUF_RT_REFL), want[f]["refl"]) and np.array_equal(o.buffer(O.BUF_RT_DIFF), want[f]["diff"]), f
            assert rays == want[f]["rays"] and o.light_rays == want[f]["light_rays"] > 0, f
            assert (o.pick_wf[o.pick_info[..., 1] != LP.NONE, 1] == 1.0).all()
        assert o.seq == 4
        v = o.images[0]["v"][..., 1]      # s = 4 wrote image 0
        assert (v < 128).any() and (v == 255).any()      # three or four occlusions in a row; lit throughout
    finally:
        o.close()


def test_the_restatement_refuses_other_values():
    o = LV.Oracle(16, 16)
    try:
        o.set_light_pick_visibility(1)
        for bad in (2, -1, True):
            with pytest.raises(ValueError):
                o.set_light_pick_visibility(bad)
        assert o.light_vis is True
    finally:
        o.close()


# ---- the update ---------------------------------------------------------------------------------------------------------------------------
def test_the_update_table():
    """All 256 values and both outcomes against Python integers; 0 and 255 fixed points, reached exactly; monotone in v and toward the
    outcome; how many outcomes of a kind in a row cross the whole range (the restatement counts them)."""
    for occluded in (False, True):
        table = [LV.update_lib(v, occluded) for v in range(256)]
        assert table == [LV.update(v, occluded) for v in range(256)]
        assert all(0 <= x <= 255 for x in table)
        assert all(a <= b for a, b in zip(table, table[1:]))      # monotone in v
        if occluded:
            assert table[0] == 0 and all(table[v] < v for v in range(1, 256))
        else:
            assert table[255] == 255 and all(table[v] > v for v in range(255))
    down, up = LV.runs()
    print("the update: %d occlusions in a row from 255 to 0, %d lit outcomes from 0 to 255" % (down, up))
    # The rule's integers, counted: sixteen outcomes of a kind leave the byte one code short of the end (1, 254), the seventeenth reaches it.
    # (The feature's description says sixteen; the formula is what is restated bit for bit, and these are its counts.)
    assert (down, up) == (17, 17)
    v, w, steps = 255, 0, []
    for _ in range(17):
        v, w = LV.update(v, True), LV.update(w, False); steps.append((v, w))
    assert steps[15] == (1, 254) and steps[16] == (0, 255), steps
    assert steps[9][0] < LV.FLOOR <= steps[8][0], steps      # below the floor after the tenth occlusion


# ---- the draw on weighted candidates ----------------------------------------------------------------------------------------------------------
PATTERNS = np.array([[255, 255, 255, 255, 255, 255, 255, 255], [3, 255, 255, 0, 0, 0, 0, 0], [255, 16, 17, 1, 1, 1, 1, 1], [64, 200, 128, 9, 9, 9, 9, 9],
                     [255, 0, 255, 7, 7, 7, 7, 7], [15, 15, 15, 0, 0, 0, 0, 0], [128, 255, 40, 2, 2, 2, 2, 2], [200, 100, 50, 5, 5, 5, 5, 5]], np.uint8)


def standing(lights=HARD, vis=1):
    """An oracle of the golden scene whose camera and model stand (velocity 0): one frame traced without the setting's pass acting.
    (oracle, base frame index)."""
    o = LV.Oracle(W, H)
    HS.scene(o, metallic=MIXED)
    eye = (10.0, 10.0, -24.0)
    o.camera_frame(eye, 0.0)      # (no lights yet: the frame's own velocity words are zero from here on)
    o.set_lights(lights); o.set_light_sampling(1); o.set_light_pick_visibility(vis)
    return o, HS.frame_index(o)


def overwrite(o, v):
    """The image the next pass reads, overwritten: bytes `v` [H, W, 8], this frame's normal words, the stamp of frame s - 1 and the pixel's
    instance -- valid history for a standing camera."""
    img = o.images[(o.seq - 1) & 1]
    vis = o.buffer(O.BUF_VISIBILITY).reshape(o.H, o.W).astype(np.int64)
    img["v"] = v
    img["normal"] = o.buffer(O.BUF_NORMAL).reshape(o.H, o.W)
    img["stamp"] = ((((o.seq - 1) & 0xFFFFFF) << 8) | np.where(vis > 0, ((vis - 1) >> 24) + 1, 0)).astype(np.uint32)


def test_the_values_of_the_draw_that_choose_a_light_form_one_interval_of_its_weighted_share():
    """Eight pixels with hand-set bytes (PATTERNS: below the floor, at it, above, at 0 and 255): U and the chosen light of the walker are
    those of u = w max(v, 16); all 2^24 values of v >> 8 choose each light over one interval, in the lights' order, of its share u_i / U."""
    o, base = standing()
    try:
        HS.set_frame_index(o, base); o.ray_trace()      # s = 1
        y, x = np.mgrid[0:H, 0:W]
        which = (x + 3 * y) % 8
        o.scramble = lambda oo: overwrite(oo, PATTERNS[which])
        HS.set_frame_index(o, base + 1); o.lights_apply()      # s = 2: the history is valid where it is the pixel's own
        cls, n = o.vis_info[..., 0], o.pick_info[..., 0].astype(int)
        assert (cls[n > 0] == LV.VALID).all()
        done = 0
        for k in range(8):
            pixels = np.argwhere((which == k) & (n >= 2))
            assert len(pixels), k
            py, px = pixels[len(pixels) // 2]
            w, v = o.pick_weights[py, px], PATTERNS[k]
            u = LV.weighted(w, v)
            cand = w > 0
            U = np.float32(0.0)
            for i in range(8):
                if cand[i]:
                    U = np.float32(U + u[i])
            assert U == o.pick_wf[py, px, 0], (k, U, o.pick_wf[py, px])
            got = LP.intervals(u)
            assert sum(c for c, _, _ in got) == 1 << 24
            at, draw = 0, LP.draw_word(int(py) * W + int(px), base + 1, LP.PICK_SLOT) >> 8
            for i, (count, first, last) in enumerate(got):
                if not cand[i]:
                    assert count == 0, (k, i)
                    continue
                assert count > 0 and first == at and last - first + 1 == count, (k, i, got)
                at = last + 1
                share = float(u[i]) / float(U)
                assert abs(count / float(1 << 24) - share) <= 2.0 ** -22, (k, i, count, share)
                if first <= draw <= last:
                    assert o.pick_info[py, px, 1] == i, (k, i)
                    assert o.pick_wf[py, px, 1] == np.float32(U / u[i])
            done += 1
        assert done == 8 and (PATTERNS[1][0] < LV.FLOOR)
    finally:
        o.close()


# ---- the estimator ----------------------------------------------------------------------------------------------------------------------
def mode0_sum(lights):
    """Mode 0's S in fp32 at radius 0: a light alone in mode 1 is that light's term of mode 0 (f = 1, no hash), added in index order."""
    S = np.zeros((H, W, 6), np.float32)
    for i in range(len(lights)):
        alone = [dict(l, intensity=l["intensity"] if k == i else [0.0, 0.0, 0.0]) for k, l in enumerate(lights)]
        o, base = standing(alone, vis=0)
        HS.set_frame_index(o, base); o.ray_trace()
        S = S + o.pick_terms
        o.close()
    return S


def run(vis, frames, scrambled=False, marks=(64, 256)):
    """`frames` frames of the standing golden scene at radius 0 in mode 1, with or without the setting: the relative L2, over the pixels that
    have a term in mode 0, of the mean of the fp32 terms against mode 0's S after each of `marks` frames; and over frames 16 .. 63 the
    traced shadow rays and how many came back unoccluded."""
    S = mode0_sum(HARD)
    has = S.any(-1)
    o, base = standing(HARD, vis=vis)
    try:
        if scrambled:
            rng = np.random.default_rng(20261021)
            o.scramble = lambda oo: overwrite(oo, rng.integers(0, 256, (H, W, 8), dtype=np.uint8))
        total, err, lit, occluded = np.zeros((H, W, 6), np.float64), {}, 0, 0
        for f in range(frames):
            HS.set_frame_index(o, base + f)
            o.ray_trace() if f == 0 else o.lights_apply()
            total += o.pick_terms
            if 16 <= f < 64:
                lit += int((o.pick_info[..., 2] == LR.LIT).sum()); occluded += int((o.pick_info[..., 2] == LR.OCCLUDED).sum())
            if f + 1 in marks:
                mean = total / (f + 1)
                err[f + 1] = float(np.sqrt(((mean - S)[has] ** 2).sum() / (S[has].astype(np.float64) ** 2).sum()))
            if vis and f >= 1:
                assert o.acted and ((o.vis_info[..., 0] == LV.VALID) == (o.vis_info[..., 0] != LV.NOT_COVERED)).all()      # standing: every covered pixel has its history
        return err, lit, occluded, int(has.sum())
    finally:
        o.close()


def occluded_share(lights):
    """Of the chosen rays of mode 1's restatement over frames 0 .. 63 of the still scene, the share that is occluded."""
    o = LP.Oracle(W, H)
    try:
        HS.scene(o, metallic=MIXED)
        o.set_lights(lights); o.set_light_sampling(1)
        base, lit, occ = HS.frame_index(o), 0, 0
        for f in range(64):
            HS.set_frame_index(o, base + f)
            o.ray_trace() if f == 0 else o.lights_apply()
            lit += int((o.pick_info[..., 2] == LR.LIT).sum()); occ += int((o.pick_info[..., 2] == LR.OCCLUDED).sum())
        return occ / float(occ + lit)
    finally:
        o.close()


def test_the_scene_wastes_a_quarter_of_mode_1s_rays():
    """A condition on the reference alone, checked first: lights_classes.json's mesh, camera and materials, and lights of which mode 1 finds at
    least a quarter of its chosen rays occluded."""
    assert {k: GOLDEN[k] for k in ("width", "height", "metallic", "spot_degrees")} == {
        k: json.load(open(os.path.join(HS.ROOT, "tests", "golden", "lights_classes.json")))[k] for k in ("width", "height", "metallic", "spot_degrees")}
    share, hard = occluded_share(LIGHTS), occluded_share(HARD)
    print("mode 1, frames 0 .. 63: %.4f of the chosen rays are occluded (radius 0: %.4f)" % (share, hard))
    assert share >= 0.25 and hard >= 0.25
    assert abs(share - GOLDEN["mode1_occluded_share"]) <= 1e-12 and abs(hard - GOLDEN["mode1_occluded_share_radius0"]) <= 1e-12, (share, hard)


@pytest.mark.parametrize("scrambled", [False, True], ids=["the history as it comes", "the history overwritten with arbitrary bytes"])
def test_the_mean_over_frames_converges_to_mode_0(scrambled):
    """An unbiased estimator halves its error from 64 to 256 frames; a biased one plateaus (the bar of tests/test_light_pick_host.py).  The
    second run overwrites the image read in front of every frame -- valid stamps, random bytes: history cannot bias."""
    err, _, _, pixels = run(1, 256, scrambled)
    key = "convergence_scrambled" if scrambled else "convergence"
    print("%s: %d pixels, relative L2 %.5f after 64 frames, %.5f after 256, ratio %.3f" % (key, pixels, err[64], err[256], err[256] / err[64]))
    assert pixels > 2000
    assert err[256] < 0.7 * err[64], err
    assert abs(err[64] - GOLDEN[key]["frames64"]) <= 1e-9 and abs(err[256] - GOLDEN[key]["frames256"]) <= 1e-9, err


def test_it_helps_where_mode_1_wastes_rays():
    """The standing scene, frames 16 .. 63: more of the traced shadow rays come back unoccluded than in mode 1, and the error of the mean
    after 64 frames is not above mode 1's.  No margin beyond "better than the parent's mode"."""
    e1, lit1, occ1, _ = run(0, 64, marks=(64,))
    ev, litv, occv, _ = run(1, 64, marks=(64,))
    s1, sv = lit1 / float(lit1 + occ1), litv / float(litv + occv)
    print("unoccluded share of the traced shadow rays, frames 16 .. 63: mode 1 %.4f, with the records %.4f; relative L2 after 64 frames: %.5f, %.5f" % (s1, sv, e1[64], ev[64]))
    assert sv > s1, (sv, s1)
    assert ev[64] <= e1[64], (ev, e1)
    g = GOLDEN["helps"]
    assert abs(s1 - g["mode1_unoccluded_share"]) <= 1e-12 and abs(sv - g["unoccluded_share"]) <= 1e-12 and abs(e1[64] - g["mode1_frames64"]) <= 1e-9 and abs(ev[64] - g["frames64"]) <= 1e-9


# ---- the class conditions -------------------------------------------------------------------------------------------------------------------
def camera(f):
    """The golden camera: it moves for six frames (the model turning), stands, and jumps."""
    c = GOLDEN["camera"]
    if f < c["moving"]:
        return tuple(c["eye"][k] + c["step"][k] * f for k in range(3)), c["dt"]
    if f < c["jump_at"]:
        return tuple(c["eye"][k] + c["step"][k] * (c["moving"] - 1) for k in range(3)), 0.0
    return tuple(c["jump_to"]), 0.0


def class_frames():
    c = GOLDEN["camera"]
    o = LV.Oracle(W, H)
    try:
        HS.scene(o, metallic=MIXED)
        o.set_lights(LIGHTS); o.set_light_sampling(1); o.set_light_pick_visibility(1)
        frames = []
        for f in range(c["frames"]):
            if f == c["set_lights_at"]:
                o.set_lights(LIGHTS)      # the same list: a reset all the same
            o.camera_frame(*camera(f))
            frames.append(LV.counts(o))
        return frames
    finally:
        o.close()


def test_the_class_conditions_of_a_camera_that_moves_stands_and_jumps():
    frames = class_frames()
    c = GOLDEN["camera"]
    print("classes: %s" % LV.total(frames))
    LV.check_conditions(frames, "golden")
    assert frames[0]["valid"] == 0 and frames[0]["sequence"] > 0 and frames[1]["valid"] > 0
    after = frames[c["set_lights_at"]]      # the frame after an rtggx_set_lights has no valid history anywhere
    assert after["valid"] == 0 and after["sequence"] > 0 and sum(after[k] for k in ("off_frame", "stamp", "instance", "normal")) == 0
    assert frames[c["set_lights_at"] + 1]["valid"] > 0
    assert frames[c["jump_at"]]["off_frame"] > 0
    assert LV.total(frames) == GOLDEN["classes"], LV.total(frames)
    assert frames == GOLDEN["class_frames"]
