"""A light list beyond eight, the part that needs no GPU: rtggx_set_light_list, rtggx_read_light_list_counts and
rtggx_debug_light_list_cull declared, exported and bound, and the header's rule; -lightlist checked at parse time; the restatement
(tests/light_list_ref.cpp) with a list of eight lights or fewer against tests/light_pick_ref.cpp's mode 1; the hash slots worked out apart
from it; the class conditions of the scene and the list the GPU tests use (tests/golden/light_list_classes.json); and unbiasedness: the
mean of the picks converges to the sum over all lights, each behind a ray of its own.

    python tests/test_light_list_host.py --write-golden

writes tests/golden/light_list_classes.json: the list from GOLDEN_SEED and the figures the restatement gives for it."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import host_support as HS
import light_list_ref as LL
import light_pick_ref as LP
import lights_ref as LR
from oracle import oracle as O

GOLDEN_PATH = os.path.join(HS.ROOT, "tests", "golden", "light_list_classes.json")
PICK = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "light_pick_classes.json")))      # the scene: 148 x 84, mixed materials
W, H, MIXED, FRAMES = PICK["width"], PICK["height"], tuple(PICK["metallic"]), PICK["frames"]
GOLDEN_SEED, GOLDEN_LIGHTS = 20261021, 96
SPOT_DEGREES = (35.0, 20.0)


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def golden_lights(seed=GOLDEN_SEED):
    """96 lights for the 148 x 84 scene (the ground slab over x, z in [-10, 10] at y = 0, the model above its middle up to y = 9.8):
    0 .. 63 an 8 x 8 lattice of small-range point lights over the ground; 64 .. 94 three rings of small-range lights around the model;
    95 one light whose range covers everything.  Four of the rings' lights have a cone toward the model, twelve lights a radius (eleven of
    them low over the ground, where a target can lie below the horizon), four no intensity -- one below index 8, two above 64."""
    rng = np.random.RandomState(seed)
    r3 = lambda x: float(np.round(x, 3))
    lights = []
    for iz in range(8):
        for ix in range(8):
            lights.append(dict(position=[r3(-8.75 + 2.5 * ix + rng.uniform(-0.4, 0.4)), r3(rng.uniform(0.9, 1.6)), r3(-8.75 + 2.5 * iz + rng.uniform(-0.4, 0.4))],
                               intensity=[r3(rng.uniform(5.0, 9.0)), r3(rng.uniform(5.0, 9.0)), r3(rng.uniform(4.0, 8.0))], range=r3(rng.uniform(3.0, 3.8))))
    for k in range(31):
        ring, angle = k % 3, 2.0 * np.pi * (k // 3) / 11.0 + 0.2 * (k % 3)
        radius = rng.uniform(5.4, 6.4)
        lights.append(dict(position=[r3(radius * np.cos(angle)), r3((2.0, 5.0, 8.0)[ring] + rng.uniform(-0.5, 0.5)), r3(radius * np.sin(angle))],
                           intensity=[r3(rng.uniform(8.0, 14.0)), r3(rng.uniform(8.0, 14.0)), r3(rng.uniform(8.0, 14.0))], range=r3(rng.uniform(4.0, 5.0))))
    lights.append(dict(position=[6.0, 14.0, -12.0], intensity=[60.0, 60.0, 70.0], range=60.0))
    for i in (10, 13, 18, 21, 27, 34, 36, 42, 45, 50, 53):      # low over the ground, with a radius
        lights[i]["position"][1] = 0.4
        lights[i]["radius"] = 0.5
    lights[66]["radius"] = 0.4
    cos_outer, cos_inner = LR.cone(*SPOT_DEGREES)
    for i in (68, 74, 80, 86):      # a cone toward the model
        p = lights[i]["position"]
        lights[i].update(axis=[r3(-p[0]), r3(4.0 - p[1]), r3(-p[2])], cos_outer=cos_outer, cos_inner=cos_inner, range=9.0)
        lights[i]["intensity"] = [r3(4.0 * x) for x in lights[i]["intensity"]]
    for i in (3, 40, 70, 90):       # no intensity: they keep their index and cast nothing
        lights[i]["intensity"] = [0.0, 0.0, 0.0]
    assert len(lights) == GOLDEN_LIGHTS
    return lights


def list_file_lines(lights, spot_degrees=SPOT_DEGREES):
    """The lines of a -lightlist file for `lights`: light for a light without a cone, spot (with the half-angles in degrees) for one with."""
    out = ["# %d lights" % len(lights), ""]
    for l in lights:
        head = list(l["position"]) + list(l["intensity"]) + [l["range"]]
        if "cos_outer" in l:
            out.append("spot " + " ".join(repr(float(x)) for x in head + [l.get("radius", 0.0)] + list(l["axis"]) + list(spot_degrees)))
        else:
            out.append("light " + " ".join(repr(float(x)) for x in head + ([l["radius"]] if "radius" in l else [])) + "   # a point light")
    return out


def oracle(lights, depth=1, samples=1, reflections=False, sun=False, size=None):
    o = LL.Oracle(*(size or (W, H)), depth=depth, samples=samples)
    HS.scene(o, metallic=MIXED)
    if sun:
        o.set_sun([-0.6, 0.5, -0.3], [3.0, 3.0, 3.0]); o.set_sun_reflections(True); o.set_sun_angle(5.0)
    o.set_light_list(lights)
    o.set_light_reflections(1 if reflections else 0)
    return o


def golden_figures(lights, depth):
    """The figures of `lights` over the first FRAMES frame indices of the still scene, at depth 1 or at depth 2 with the lights at the hits."""
    o = oracle(lights, depth=depth, reflections=depth >= 2)
    try:
        base = HS.frame_index(o)
        frames, both = [], []
        for f in range(FRAMES):
            HS.set_frame_index(o, base + f)
            o.ray_trace()
            frames.append(LL.record(o))
            chunks = LL.block_kept_chunks(o)
            both.append(chunks.all(0) if len(chunks) >= 2 else np.zeros(chunks.shape[1:], bool))
        return LL.figures(frames, LL.casting(lights), both, depth >= 2)
    finally:
        o.close()


def convergence(lights):
    """`lights` with every radius 0, where the sum over the lights is deterministic: the relative L2 error, over the pixels that have a
    term, of the mean of the picks' fp32 terms over frames 0 .. 63 and over frames 0 .. 255 against S, every light behind a ray of its own."""
    lights = [dict(l, radius=0.0) for l in lights]
    o = oracle(lights)
    try:
        base = HS.frame_index(o)
        o.lights_apply(sum_all=True)
        S = o.list_terms.copy()
        has = S.any(-1)
        total, err = np.zeros((H, W, 6), np.float64), {}
        for f in range(256):
            HS.set_frame_index(o, base + f)
            o.lights_apply()
            total += o.list_terms
            if f + 1 in (64, 256):
                mean = total / (f + 1)
                err[f + 1] = float(np.sqrt(((mean - S)[has] ** 2).sum() / (S[has].astype(np.float64) ** 2).sum()))
        return err[64], err[256], int(has.sum())
    finally:
        o.close()


def write_golden():
    lights = golden_lights()
    e64, e256, pixels = convergence(lights)
    prefix = golden_figures(lights[:65], 1)
    out = dict(width=W, height=H, metallic=list(MIXED), frames=FRAMES, seed=GOLDEN_SEED, spot_degrees=list(SPOT_DEGREES), columns=list(LL.COLUMNS),
               lights=lights, depth1=golden_figures(lights, 1), depth2=golden_figures(lights, 2),
               prefix65=dict(none_kept=prefix["blocks"]["none_kept"], covered=prefix["blocks"]["covered"]),
               convergence=dict(frames64=e64, frames256=e256, pixels=pixels))
    with open(GOLDEN_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("depth1", "depth2", "prefix65", "convergence")}, indent=1))


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-golden"]:
        write_golden()
    sys.exit(0)

GOLDEN = json.load(open(GOLDEN_PATH))
LIGHTS = GOLDEN["lights"]


# ---- declared, exported, bound ---------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound(built):
    HS.declared_exported_bound(
        "rtggx_set_light_list", r"\bint\s+rtggx_set_light_list\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*const\s+RtggxLight\s*\*\s*lights\s*,\s*uint32_t\s+count\s*\)",
        defines=(r"#define\s+RTGGX_MAX_LIGHT_LIST\s+1024u", r"#define\s+RTGGX_MAX_LIGHTS\s+8u", r"typedef struct RtggxLight \{\s+/\* 64 bytes \*/",
                 r"is mode 1's rule, whatever rtggx_set_light_sampling says", r"with i\s+\*?\s*running 0 \.\. n - 1",
                 r"16 \+ i for i < 8, 4096 \+ i for i >= 8", r"32 \+ 16 d \+ 8 img \+ i for i < 8, 8192 \+ 1024 \(2 d \+ img\) \+ i for i >= 8",
                 r"e_c = max\(max\(lo_c - Pl_c, Pl_c - hi_c\), 0\)", r"dist2 = \(e_x e_x \+ e_y e_y\) \+ e_z e_z", r"RRm = \(R R\) 1\.000244140625f",
                 r"light k is KEPT iff dist2 < RRm", r"A light without intensity is never kept", r"d2 < R R at any pixel implies\s+\*?\s*dist2 < R R \(1 \+ 2\^-20\) < RRm",
                 r"the context holds one or the other", r"rtggx_set_light_pick_visibility does not act on a list", r"It does not act on a light list \(rtggx_set_light_list\)",
                 r"no culling by cone or by facing", r"no more than 1024 lights"),
        method="set_light_list")
    HS.declared_exported_bound("rtggx_read_light_list_counts", r"\bint\s+rtggx_read_light_list_counts\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*uint32_t\s*\*\s*out\s*,\s*size_t\s+bytes\s*\)")
    HS.declared_exported_bound("rtggx_debug_light_list_cull", r"\bint\s+rtggx_debug_light_list_cull\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*int\s+enable\s*\)")
    from raytracedggx_amd import app, capi
    L = capi.load()
    assert L.rtggx_set_light_list.argtypes == [C.c_void_p, C.POINTER(capi.Light), C.c_uint32]
    assert L.rtggx_read_light_list_counts.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t] and L.rtggx_debug_light_list_cull.argtypes == [C.c_void_p, C.c_int]
    assert C.sizeof(capi.Light) == 64 and capi.MAX_LIGHTS == 8 and capi.MAX_LIGHT_LIST == 1024 == LL.MAX_LIGHT_LIST
    assert "rtggx_app_set_light_list" in app.HOST_EXPORTS and hasattr(C.CDLL(app.HOST_LIB_PATH), "rtggx_app_set_light_list")
    assert callable(getattr(app.RayTracedGGX, "set_light_list", None))
    for name in ("RayTracedGGX.h", "RayTracedGGX.cpp"):      # the flag list and kFlags
        text = open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", name)).read()
        assert "-lightlist" in text or '"lightlist"' in text
    assert "SetLightList" in open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", "RayTracer.h")).read()
    header = open(os.path.join(HS.ROOT, "include", "rtggx.h")).read()
    struct = re.search(r"typedef struct RtggxLight \{(.*?)\} RtggxLight;", header, re.S).group(1)
    assert re.findall(r"float\s+(\w+)(?:\[(\d)\])?;", struct) == [("position", "3"), ("range", ""), ("intensity", "3"), ("radius", ""), ("axis", "3"), ("cos_outer", ""),
                                                                ("cos_inner", ""), ("pad", "3")]


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def write_list(path, lines):
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)


def test_the_executable_refuses_a_bad_list_before_asking_for_a_device(built, tmp_path):
    good = write_list(tmp_path / "good.txt", list_file_lines(LIGHTS[:12] + [LIGHTS[68]]))
    bad = write_list(tmp_path / "bad.txt", ["# a list", "light 0 1 0 1 1 1 5", "", "light 0 1 0 1 1 1 -5   # a negative range"])
    word = write_list(tmp_path / "word.txt", ["light 0 1 0 1 1 1 5", "lamp 0 1 0 1 1 1 5"])
    short = write_list(tmp_path / "short.txt", ["light 0 1 0 1 1 1 5", "light 0 1 0 1 1 1 5", "spot 0 1 0 1 1 1 5 0 0 -1 0 30"])
    many = write_list(tmp_path / "many.txt", ["light %d 1 0 1 1 1 5" % i for i in range(1025)])
    HS.executable_refuses([
        (["-lightlist", str(tmp_path / "missing.txt")], "cannot open"), (["-lightlist"], "-lightlist"),
        (["-lightlist", bad], "line 4"), (["-lightlist", word], "line 2"), (["-lightlist", short], "line 3"),
        (["-lightlist", many], "at most 1024"), (["-lightlist", many], "line 1025"),
        (["-lightlist", good, "-light", "1", "2", "3", "4", "5", "6", "7"], "-lightlist together with -light"),
        (["-spot", "1", "2", "3", "4", "5", "6", "9", "0.5", "0", "-1", "0", "30", "20", "-lightlist", good], "-lightlist together with -light"),
        (["-lightlist", good, "-rayrate", "4"], "-rayrate 4"), (["-rayrate", "4", "-lightlist", good], "-rayrate 4"),
        (["-lightpick", "-lightlist", good], "-lightpick"), (["-lightvisibility", "-lightlist", good], "-lightvisibility"),
        (["-lightreflections"], "-lightreflections")])


def test_the_executable_parses_a_good_list(built, tmp_path):
    """What stops these runs is the environment file, which is read after the command line and before a device is asked for."""
    import assets
    good = write_list(tmp_path / "good.txt", list_file_lines(LIGHTS))
    full = write_list(tmp_path / "full.txt", ["light %d 1 0 1 1 1 5" % i for i in range(1024)])
    missing = str(tmp_path / "missing.hdr")
    HS.executable_refuses([["-env", missing, "-lightlist", good], ["-env", missing, "-lightlist", full, "-lightreflections", "-recursion", "2"],
                           ["-env", missing, "-lightreflections", "-lightlist", good, "-sun", "0", "1", "0", "1", "1", "1", "-sunreflections"]],
                          must_mention="cannot open", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
SHORT = PICK["lights"] + [LIGHTS[95], LIGHTS[3], LIGHTS[27], LIGHTS[66], LIGHTS[68]]      # eight: a cone, radii, one without intensity


@pytest.mark.parametrize("depth,samples", [(1, 1), (2, 2)], ids=["depth 1", "depth 2, N = 2, the lights at the hits"])
def test_a_list_of_eight_is_light_pick_refs_mode_1(depth, samples):
    """Below index 8 the slots of rtggx_set_lights hold: images and ray counts are tests/light_pick_ref.cpp's, bit for bit."""
    assert len(SHORT) == 8
    p = LP.Oracle(W, H, depth=depth, samples=samples)
    o = oracle(SHORT, depth=depth, samples=samples, reflections=depth >= 2)
    try:
        HS.scene(p, metallic=MIXED)
        p.set_lights(SHORT); p.set_light_reflections(1 if depth >= 2 else 0); p.set_light_sampling(1)
        for f in range(2):
            for x in (p, o):
                HS.set_frame_index(x, HS.frame_index(x) + f)
            want, got = p.ray_trace(), o.ray_trace()
            assert got == want and o.light_rays == p.light_rays > 0 and o.light_hit_rays == p.light_hit_rays
            for b in (O.BUF_RT_REFL, O.BUF_RT_DIFF, O.BUF_NORMAL, O.BUF_ROUGH_METAL, O.BUF_VELOCITY):
                assert np.array_equal(o.buffer(b), p.buffer(b)), (f, b)
            chosen = np.where(p.pick_info[..., 1] == LP.NONE, LL.NONE, p.pick_info[..., 1].astype(np.uint16))
            assert np.array_equal(o.list_info[..., 1], chosen) and (chosen != LL.NONE).sum() > 2000
            assert np.array_equal(o.list_terms, p.pick_terms) and np.array_equal(o.list_wf, p.pick_wf)
            if depth >= 2:
                assert p.light_hit_rays > 0 and np.array_equal(o.list_chosen0, p.pick_chosen0.astype(np.int16))
    finally:
        p.close(); o.close()


def test_the_restatement_holds_lights_or_a_list():
    o = LL.Oracle(16, 16)
    try:
        o.set_light_list(SHORT)
        with pytest.raises(ValueError):
            o.set_lights(SHORT[:1])
        o.set_lights([])
        with pytest.raises(ValueError):
            o.set_light_list([dict(position=[0, 1, 0], intensity=[1, 1, 1], range=5.0)] * 1025)
        assert len(o.light_list) == 8
        o.set_light_list(None); o.set_lights(SHORT[:1])
        with pytest.raises(ValueError):
            o.set_light_list(SHORT)
        o.set_light_list([])
    finally:
        o.close()


def test_the_slots_worked_out_by_hand():
    """i = 7, 8 and 1023 from Python integers against the restatement's; above 7 the slots meet nothing in use."""
    L = LL.lib()
    assert [LL.slot(i) for i in (7, 8, 1023)] == [23, 4104, 5119] == [int(L.orc_light_list_slot(i)) for i in (7, 8, 1023)]
    for d in range(4):
        for img in range(2):
            want = [32 + 16 * d + 8 * img + 7, 8192 + 1024 * (2 * d + img) + 8, 8192 + 1024 * (2 * d + img) + 1023]
            assert [LL.hit_slot(d, img, i) for i in (7, 8, 1023)] == want == [int(L.orc_light_list_hit_slot(d, img, i)) for i in (7, 8, 1023)]
    in_use = set(range(0, 9)) | set(range(16, 24)) | set(range(32, 96)) | {96} | set(range(104, 112))
    new = {LL.slot(i) for i in range(8, 1024)} | {LL.hit_slot(d, img, i) for d in range(4) for img in range(2) for i in range(8, 1024)}
    assert len(new) == 1016 * 9 and not new & in_use
    assert {LL.slot(i) for i in range(8)} == set(range(16, 24)) and {LL.hit_slot(d, img, i) for d in range(4) for img in range(2) for i in range(8)} == set(range(32, 96))


# ---- the class conditions of the scene and the list the GPU tests use --------------------------------------------------------------------------
def test_the_golden_list_is_the_generators():
    assert LIGHTS == golden_lights(GOLDEN["seed"]) and len(LIGHTS) == GOLDEN_LIGHTS == 96
    assert {k: GOLDEN[k] for k in ("width", "height", "metallic", "frames")} == {k: PICK[k] for k in ("width", "height", "metallic", "frames")}
    assert GOLDEN["columns"] == list(LL.COLUMNS) and GOLDEN["spot_degrees"] == list(SPOT_DEGREES)
    dark = [i for i, l in enumerate(LIGHTS) if not any(l["intensity"])]
    assert len(dark) >= 4 and min(dark) < 8 and max(dark) > 64
    assert sum(1 for l in LIGHTS if "cos_outer" in l) >= 4 and sum(1 for l in LIGHTS if l.get("radius", 0) > 0) >= 4
    assert LIGHTS[95]["range"] >= 60.0      # the scene lies within 40 of it


@pytest.mark.parametrize("depth", [1, 2], ids=["depth 1", "depth 2, the lights at the hits"])
def test_the_class_conditions_of_the_scene_the_gpu_tests_use(depth):
    """Over the first FRAMES frame indices of the still scene the conditions hold on the restatement alone, and the figures are the golden
    file's.  One light's range covers everything, so every block with a covered pixel keeps it: the blocks that keep nothing are those of
    the list's first 65 lights, which the GPU tests run as a list of their own."""
    got = golden_figures(LIGHTS, depth)
    print(got)
    assert got == GOLDEN["depth%d" % depth], got
    assert ("hits" in got) == (depth >= 2)
    assert got["blocks"]["none_kept"] == 0
    if depth == 1:
        prefix = golden_figures(LIGHTS[:65], 1)
        assert prefix["blocks"]["none_kept"] == GOLDEN["prefix65"]["none_kept"] and prefix["blocks"]["covered"] == GOLDEN["prefix65"]["covered"]
        got = dict(got, blocks=dict(got["blocks"], none_kept=prefix["blocks"]["none_kept"]))
    else:
        got = dict(got, blocks=dict(got["blocks"], none_kept=GOLDEN["prefix65"]["none_kept"]))
    LL.check_conditions(got, "golden, depth %d" % depth)


def test_the_mean_over_frames_converges_to_the_sum_over_all_lights():
    """An unbiased estimator halves its error from 64 to 256 frames; a biased one plateaus.  The bar of tests/test_light_pick_host.py."""
    e64, e256, pixels = convergence(LIGHTS)
    print("convergence: %d pixels, relative L2 %.5f after 64 frames, %.5f after 256" % (pixels, e64, e256))
    assert pixels > 2000
    assert e256 <= 0.7 * e64, (e64, e256)
    assert abs(e64 - GOLDEN["convergence"]["frames64"]) <= 1e-9 and abs(e256 - GOLDEN["convergence"]["frames256"]) <= 1e-9, (e64, e256)
