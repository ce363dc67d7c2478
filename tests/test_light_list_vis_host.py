"""A list's pick weighted by what the pixel remembers, the part that needs no GPU: rtggx_set_light_list_visibility and
rtggx_read_light_list_visibility declared, exported and bound, the record's 16 bytes, -lightlistvisibility checked at parse time; the
restatement (tests/light_list_vis_ref.cpp) against tests/light_list_ref.cpp's frames with the setting off and with one casting light; the
update's rule against Python integers; the floor and the scale of the remembered values (test A); convergence to the sum over all lights
with the history as it comes and with both record images overwritten by arbitrary bytes (test B); that it helps on a scene whose brightest
lamps stand behind the model (test C); and the class conditions of a camera that stands, moves and jumps
(tests/golden/light_list_vis_classes.json).

    python tests/test_light_list_vis_host.py --write-golden

writes tests/golden/light_list_vis_classes.json: the list from GOLDEN_SEED and the figures the restatement gives for it."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import host_support as HS
import light_list_ref as LL
import light_list_vis_ref as LV
import lights_ref as LR
from oracle import oracle as O

GOLDEN_PATH = os.path.join(HS.ROOT, "tests", "golden", "light_list_vis_classes.json")
LIST = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "light_list_classes.json")))      # the scene: 148 x 84, mixed materials, and its lattice
W, H, MIXED = LIST["width"], LIST["height"], tuple(LIST["metallic"])
GOLDEN_SEED = 20261021
# The golden camera: it stands for STILL frames (the model does not turn), then orbits for MOVING - 1 frames with the model turning, and
# jumps in the last one -- the jump is what puts reprojected taps outside the frame.
CAMERA = dict(eye=[10.0, 10.0, -24.0], step=[0.8, 0.2, 0.5], dt=0.25, still=18, moving=6, jump_to=[-12.0, 9.0, -22.0])


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def golden_lights(seed=GOLDEN_SEED):
    """73 lights for the 148 x 84 scene (the camera looks from (10, 10, -24): "behind the model" is toward -x, +z): 0 .. 63 the lattice of
    small-range lamps over the ground of light_list_classes.json, the first chunk; 64 .. 69 six bright lamps close together low behind the
    model, whose shadows on the ground in front of it overlap -- more hidden lights at a pixel than a record has entries; 70, 71 two more
    to the sides; 72 one very bright lamp with a radius, range 40: wide penumbrae, and beyond the others' range pixels with one hidden
    light alone, where its v falls frame after frame."""
    rng = np.random.RandomState(seed)
    r3 = lambda x: float(np.round(x, 3))
    lights = [dict(l) for l in LIST["lights"][:64]]
    for k in range(6):
        lights.append(dict(position=[r3(-2.5 + rng.uniform(-0.8, 0.8)), r3(rng.uniform(1.5, 3.0)), r3(6.0 + rng.uniform(-0.8, 0.8))],
                           intensity=[r3(rng.uniform(300, 500))] * 3, range=r3(rng.uniform(15.0, 18.0))))
    lights.append(dict(position=[-6.5, 2.5, 3.0], intensity=[400.0, 400.0, 400.0], range=16.0))
    lights.append(dict(position=[1.5, 2.0, 7.0], intensity=[400.0, 400.0, 400.0], range=16.0))
    lights.append(dict(position=[-7.0, 3.0, 5.0], intensity=[2000.0, 2000.0, 1800.0], range=40.0, radius=1.5))
    return lights


def camera(f, c=CAMERA):
    """(eye, dt) of golden frame f."""
    if f < c["still"]:
        return tuple(c["eye"]), 0.0
    if f == c["still"] + c["moving"] - 1:
        return tuple(c["jump_to"]), c["dt"]
    return tuple(c["eye"][k] + c["step"][k] * (f - c["still"] + 1) for k in range(3)), c["dt"]


def oracle(lights, vis=1, size=None):
    o = LV.Oracle(*(size or (W, H)))
    HS.scene(o, metallic=MIXED)
    o.set_light_list(lights)
    if vis is not None:
        o.set_light_list_visibility(vis)
    return o


def class_frames(lights):
    o = oracle(lights)
    try:
        frames = []
        for f in range(CAMERA["still"] + CAMERA["moving"]):
            o.camera_frame(*camera(f))
            assert o.acted and o.seq == f + 1
            frames.append(LV.counts(o))
        return frames
    finally:
        o.close()


def standing(lights, vis):
    """An oracle of the golden scene whose camera and model stand (velocity 0 from the second frame on); (oracle, base frame index)."""
    o = oracle([], vis=None)
    o.camera_frame(tuple(CAMERA["eye"]), 0.0)
    o.set_light_list(lights); o.set_light_list_visibility(vis)
    return o, HS.frame_index(o)


def overwrite(o, entries, image=None):
    """A record image overwritten (default: the one the next pass reads): `entries` [H, W, 4], this frame's normal words, the stamp of frame
    s - 1 and the pixel's instance -- valid history for a standing camera."""
    img = o.images[(o.seq - 1) & 1 if image is None else image]
    vis = o.buffer(O.BUF_VISIBILITY).reshape(o.H, o.W).astype(np.int64)
    img["entry"] = entries
    img["normal"] = o.buffer(O.BUF_NORMAL).reshape(o.H, o.W)
    img["stamp"] = ((((o.seq - 1) & 0xFFFFFF) << 8) | np.where(vis > 0, ((vis - 1) >> 24) + 1, 0)).astype(np.uint32)


def hard(lights):
    return [dict(l, radius=0.0) for l in lights]      # radius 0, where the sum over all lights is deterministic: the estimator's tests


def run(lights, vis, frames, scrambled=False, marks=(64, 256)):
    """`frames` frames of the standing scene at radius 0, with or without the setting: the relative L2, over the pixels that have a term,
    of the mean of the picks' fp32 terms against S -- every light behind a ray of its own -- after each of `marks` frames; and over
    frames 16 .. 63 the traced shadow rays by outcome.  scrambled: BOTH record images overwritten with random bytes before every frame."""
    lights = hard(lights)
    o, base = standing(lights, vis)
    try:
        HS.set_frame_index(o, base)
        o.lights_apply(sum_all=True)
        S = o.list_terms.copy()
        has = S.any(-1)
        if scrambled:
            rng = np.random.default_rng(GOLDEN_SEED)

            def scramble(oo):
                for image in (0, 1):
                    overwrite(oo, rng.integers(0, 65536, (H, W, 4), dtype=np.uint16), image)
            o.scramble = scramble
        total, err, lit, occluded = np.zeros((H, W, 6), np.float64), {}, 0, 0
        for f in range(frames):
            HS.set_frame_index(o, base + f)
            o.lights_apply()
            total += o.list_terms
            if 16 <= f < 64:
                lit += int((o.list_info[..., 2] == LR.LIT).sum()); occluded += int((o.list_info[..., 2] == LR.OCCLUDED).sum())
            if f + 1 in marks:
                mean = total / (f + 1)
                err[f + 1] = float(np.sqrt(((mean - S)[has] ** 2).sum() / (S[has].astype(np.float64) ** 2).sum()))
        assert o.acted == bool(vis)
        return err, lit, occluded, int(has.sum())
    finally:
        o.close()


def benefit(lights):
    e0, lit0, occ0, _ = run(lights, 0, 64, marks=(64,))
    e1, lit1, occ1, _ = run(lights, 1, 64, marks=(64,))
    return dict(list_unoccluded_share=lit0 / float(lit0 + occ0), unoccluded_share=lit1 / float(lit1 + occ1), list_frames64=e0[64], frames64=e1[64])


def write_golden():
    lights = golden_lights()
    frames = class_frames(lights)
    LV.check_conditions(frames, "golden")
    e, _, _, pixels = run(lights, 1, 256)
    es, _, _, _ = run(lights, 1, 256, scrambled=True)
    out = dict(width=W, height=H, metallic=list(MIXED), seed=GOLDEN_SEED, camera=CAMERA, lights=lights, classes=LV.total(frames), class_frames=frames,
               convergence=dict(frames64=e[64], frames256=e[256], pixels=pixels), convergence_scrambled=dict(frames64=es[64], frames256=es[256]),
               helps=benefit(lights))
    with open(GOLDEN_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("classes", "convergence", "convergence_scrambled", "helps")}, indent=1))


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-golden"]:
        write_golden()
    sys.exit(0)

GOLDEN = json.load(open(GOLDEN_PATH))
LIGHTS = GOLDEN["lights"]


# ---- declared, exported, bound ---------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound(built, tmp_path):
    HS.declared_exported_bound(
        "rtggx_set_light_list_visibility", r"\bint\s+rtggx_set_light_list_visibility\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*int\s+enable\s*\)",
        defines=(r"#define\s+RTGGX_LIGHT_LIST_VIS_ENTRIES\s+4u", r"#define\s+RTGGX_LIGHT_LIST_VIS_FLOOR\s+4u", r"typedef struct RtggxLightListVisRecord",
                 r"uint16_t\s+entry\[4\];", r"\(v << 10\) \| light", r"0xFFFF: free", r"u_i = w_i \(float\)max\(v_i, RTGGX_LIGHT_LIST_VIS_FLOOR\)", r"f = U / u_i",
                 r"unoccluded v' = v \+ \(\(63 - v \+ 3\) >> 2\)", r"occluded v' = v - \(\(v \+ 3\) >> 2\)", r"\(47 << 10\) \| i", r"free slot of lowest k",
                 r"greatest v,\s+\*?\s*ties to the lowest k", r"every successful rtggx_set_light_list", r"There are no atomics", r"The cull stays invisible",
                 r"ray counts AND records", r"rtggx_debug_light_list_cull\(ctx, 0\)"),
        method="set_light_list_visibility")
    HS.declared_exported_bound(
        "rtggx_read_light_list_visibility",
        r"\bint\s+rtggx_read_light_list_visibility\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*uint32_t\s+image\s*(/\*.*?\*/)?\s*,\s*RtggxLightListVisRecord\s*\*\s*out\s*,\s*size_t\s+bytes\s*,\s*uint32_t\s*\*\s*sequence\s*\)",
        method="read_light_list_visibility")
    from raytracedggx_amd import app, capi
    L = capi.load()
    assert L.rtggx_set_light_list_visibility.argtypes == [C.c_void_p, C.c_int]
    assert L.rtggx_read_light_list_visibility.argtypes == [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    assert capi.LIGHT_LIST_VIS_RECORD.itemsize == 16 == LV.RECORD.itemsize and capi.LIGHT_LIST_VIS_FLOOR == 4 == LV.FLOOR and capi.LIGHT_LIST_VIS_ENTRIES == 4 == LV.ENTRIES
    assert [capi.LIGHT_LIST_VIS_RECORD.fields[n][1] for n in ("entry", "normal", "stamp")] == [0, 8, 12]
    src = tmp_path / "size.c"      # the header's own struct, through a C compiler
    src.write_text('#include <stddef.h>\n#include "rtggx.h"\n_Static_assert(sizeof(RtggxLightListVisRecord) == 16, "16 bytes");\n'
                   '_Static_assert(offsetof(RtggxLightListVisRecord, normal) == 8 && offsetof(RtggxLightListVisRecord, stamp) == 12, "layout");\n'
                   '_Static_assert(RTGGX_LIGHT_LIST_VIS_FLOOR == 4u && RTGGX_LIGHT_LIST_VIS_ENTRIES == 4u, "constants");\nint main(void) { return 0; }\n')
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-fsyntax-only", "-I", os.path.join(HS.ROOT, "include"), str(src)])
    assert "rtggx_app_set_light_list_visibility" in app.HOST_EXPORTS and hasattr(C.CDLL(app.HOST_LIB_PATH), "rtggx_app_set_light_list_visibility")
    assert callable(getattr(app.RayTracedGGX, "set_light_list_visibility", None))
    for name in ("RayTracedGGX.h", "RayTracedGGX.cpp"):      # the flag list and kFlags
        text = open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", name)).read()
        assert "-lightlistvisibility" in text or '"lightlistvisibility"' in text
    assert "SetLightListVisibility" in open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", "RayTracer.h")).read()


def list_file(tmp_path, lights):
    lines = ["light " + " ".join(repr(float(x)) for x in list(l["position"]) + list(l["intensity"]) + [l["range"]] + ([l["radius"]] if "radius" in l else [])) for l in lights]
    path = tmp_path / "lights.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_the_executable_refuses_the_flag_where_it_cannot_act_before_asking_for_a_device(built, tmp_path):
    good = list_file(tmp_path, LIGHTS)
    point = ["-light", "1", "2", "3", "4", "5", "6", "7"]
    HS.executable_refuses([
        (["-lightlistvisibility"], "-lightlistvisibility without -lightlist"), (["-lightlistvisibility"] + point, "-lightlistvisibility without -lightlist"),
        (["-lightlistvisibility"] + point + ["-lightpick"], "-lightlistvisibility without -lightlist"),
        (["-lightlist", good, "-lightlistvisibility", "-strips", "2"], "-lightlistvisibility: whole frames only"),
        (["-lightlistvisibility", "-lightlist", good, "-gpus", "2"], "-lightlistvisibility: whole frames only")])


def test_the_executable_parses_the_flag_with_a_list(built, tmp_path):
    """What stops these runs is the environment file, which is read after the command line and before a device is asked for."""
    import assets
    good, missing = list_file(tmp_path, LIGHTS), str(tmp_path / "missing.hdr")
    HS.executable_refuses([["-env", missing, "-lightlist", good, "-lightlistvisibility"], ["-env", missing, "-lightlistvisibility", "-lightlist", good, "-lightreflections", "-recursion", "2"]],
                          must_mention="cannot open", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
SMALL = (100, 56)


def frames_of(cls, lights, vis=None, depth=1, reflections=0, count=2, size=SMALL):
    o = cls(size[0], size[1], depth=depth)
    try:
        HS.scene(o, metallic=MIXED)
        o.set_light_list(lights); o.set_light_reflections(reflections)
        if vis is not None:
            o.set_light_list_visibility(vis)
        base, out = HS.frame_index(o), []
        for f in range(count):
            HS.set_frame_index(o, base + f)
            rays = o.ray_trace()
            out.append(dict(refl=o.buffer(O.BUF_RT_REFL), diff=o.buffer(O.BUF_RT_DIFF), rays=rays, light_rays=o.light_rays, hit_rays=o.light_hit_rays,
                            info=o.list_info.copy(), terms=o.list_terms.copy(), kept=o.list_kept.copy()))
        return out, getattr(o, "seq", None)
    finally:
        o.close()


def test_with_the_setting_off_the_frames_are_light_list_refs():
    """Never enabled, and enabled then disabled, at depth 2 with the lights at the hits; enabled, the hits still follow the list's rule: the
    hit passes' ray count is the list's."""
    want, _ = frames_of(LL.Oracle, LIGHTS, depth=2, reflections=1)
    for vis in (None, 0):
        got, seq = frames_of(LV.Oracle, LIGHTS, vis=vis, depth=2, reflections=1)
        assert seq == 0
        for f, (g, w) in enumerate(zip(got, want)):
            for k in w:
                assert np.array_equal(g[k], w[k]), (vis, f, k)
    on, seq = frames_of(LV.Oracle, LIGHTS, vis=1, depth=2, reflections=1)
    assert seq == 2 and all(g["hit_rays"] == w["hit_rays"] > 0 and np.array_equal(g["kept"], w["kept"]) for g, w in zip(on, want))
    assert want[0]["light_rays"] > 0


@pytest.mark.parametrize("radius", [0.0, 1.5], ids=["radius 0", "radius 1.5"])
def test_one_casting_light_is_the_lists_own_frame_bit_for_bit(radius):
    """Every pick is that light and f is exactly 1 whatever its entry holds: four frames equal the list's in both images and in the ray
    counts, while the entry moves.  The light is the hidden lamp, at index 72, behind 72 without an intensity."""
    lights = [dict(l, intensity=[0.0, 0.0, 0.0]) for l in LIGHTS[:72]] + [dict(LIGHTS[72], radius=radius)]
    want, _ = frames_of(LL.Oracle, lights, count=4, size=(W, H))
    o = LV.Oracle(W, H)
    try:
        HS.scene(o, metallic=MIXED)
        o.set_light_list(lights); o.set_light_list_visibility(1)
        base = HS.frame_index(o)
        for f in range(4):
            HS.set_frame_index(o, base + f)
            rays = o.ray_trace()
            assert np.array_equal(o.buffer(O.BUF_RT_REFL), want[f]["refl"]) and np.array_equal(o.buffer(O.BUF_RT_DIFF), want[f]["diff"]), f
            assert rays == want[f]["rays"] and o.light_rays == want[f]["light_rays"] > 0, f
            assert (o.list_wf[o.list_info[..., 1] != LL.NONE, 1] == 1.0).all()
        assert o.seq == 4
        e = o.images[0]["entry"]      # s = 4 wrote image 0
        held = (e != LV.FREE) & ((e & 1023) == 72)
        assert held.any() and ((e[held] >> 10) < LV.INSERT).any() and not (held.sum(-1) > 1).any()
    finally:
        o.close()


def test_the_restatement_refuses_other_values():
    o = LV.Oracle(16, 16)
    try:
        o.set_light_list_visibility(1)
        for bad in (2, -1, True):
            with pytest.raises(ValueError):
                o.set_light_list_visibility(bad)
        assert o.list_vis is True
    finally:
        o.close()


# ---- the update ---------------------------------------------------------------------------------------------------------------------------
def test_the_update_against_python_integers():
    """Every v of an existing entry in every slot, both outcomes; inserts into records with 0 .. 4 free slots; evictions with ties; a record
    that names the light twice; random records.  0 and 63 are fixed points, reached exactly, from 47 in eleven occlusions and from 0 in
    twelve lit outcomes."""
    e, F = LV.entry, LV.FREE
    cases = []
    for slot in range(4):
        for v in range(64):
            rec = [e(9, 100), e(20, 200), e(30, 300), e(40, 400)]
            rec[slot] = e(v, 1023 if v < 63 else 5)      # (v = 63 with light 1023 would be the free code)
            cases += [(rec, rec[slot] & 1023, occ) for occ in (False, True)]
    cases += [([F, F, F, F], 7, True), ([F, F, F, F], 7, False), ([e(5, 1), F, e(6, 2), F], 7, True), ([e(5, 1), e(7, 3), e(6, 2), F], 1023, True),
              ([e(5, 1), e(50, 3), e(6, 2), e(50, 4)], 7, True), ([e(47, 1), e(47, 3), e(47, 2), e(47, 4)], 0, True), ([e(0, 1), e(1, 3), e(62, 2), e(2, 4)], 9, True),
              ([e(5, 1), e(50, 3), e(6, 2), e(50, 4)], 7, False), ([e(30, 8), e(10, 8), F, e(20, 8)], 8, True), ([F, e(10, 8), e(20, 8), F], 8, False)]
    rng = np.random.default_rng(7)
    for _ in range(2000):
        rec = [int(x) for x in rng.integers(0, 65536, 4)]
        if rng.integers(0, 2):
            rec[int(rng.integers(0, 4))] = F
        light = int(rec[int(rng.integers(0, 4))] & 1023) if rng.integers(0, 2) else int(rng.integers(0, 1024))
        cases.append((rec, light, bool(rng.integers(0, 2))))
    events = set()
    for rec, light, occ in cases:
        want, got = LV.update(rec, light, occ), LV.update_lib(rec, light, occ)
        assert got == want, (rec, light, occ, got, want)
        events.add(want[1])
        assert sum(1 for a, b in zip(rec, want[0]) if a != b) <= 1      # the other slots keep the carried value
    assert events == {LV.E_KEPT, LV.E_MOVED, LV.E_INSERTED, LV.E_EVICTED, LV.E_DROPPED}
    assert LV.update([F, F, F, F], 7, True)[0] == [e(47, 7), F, F, F] and LV.update([e(5, 1), e(50, 3), e(6, 2), e(50, 4)], 7, True)[0] == [e(5, 1), e(47, 7), e(6, 2), e(50, 4)]
    assert LV.update([e(62, 7), F, F, F], 7, False)[0] == [F, F, F, F] and LV.update([e(0, 7), F, F, F], 7, True)[0] == [e(0, 7), F, F, F]
    rec, n = [F, F, F, F], 0
    while n < 100 and (n == 0 or rec[0] >> 10 != 0):
        rec, n = LV.update(rec, 7, True)[0], n + 1
    down, up = n, 0
    while up < 100 and rec[0] != F:
        rec, up = LV.update(rec, 7, False)[0], up + 1
    print("the update: %d occlusions in a row take an unrecorded light to 0, %d lit outcomes from 0 free the entry" % (down, up))
    assert (down, up) == (12, 12)


# ---- test A: the floor and the scale ----------------------------------------------------------------------------------------------------------
FOUR = [64, 66, 70, 72]      # four of the bright lamps: a list of four, so that a record can name every candidate


def four_lights():
    return hard([LIGHTS[i] for i in FOUR])


def picks(lights, entries, frames=3):
    """`frames` frames of the standing scene with every pixel's history overwritten by `entries` (None: the setting off): per frame both
    images, the chosen lights, f, and the terms."""
    o, base = standing(lights, 0 if entries is None else 1)
    try:
        if entries is not None:
            o.scramble = lambda oo: overwrite(oo, np.broadcast_to(np.array(entries, np.uint16), (H, W, 4)))
        out = []
        for f in range(frames):
            HS.set_frame_index(o, base + f)
            o.ray_trace() if f == 0 else o.lights_apply()
            out.append(dict(refl=o.buffer(O.BUF_RT_REFL), diff=o.buffer(O.BUF_RT_DIFF), chosen=o.list_info[..., 1].copy(), f=o.list_wf[..., 1].copy(), terms=o.list_terms.copy(),
                            valid=((o.vis_info[..., 0] == LV.VALID) == (o.vis_info[..., 0] != LV.NOT_COVERED)).all() if f >= 1 and entries is not None else True))
        return out
    finally:
        o.close()


def test_above_the_floor_only_the_ratios_of_the_remembered_values_count():
    """Test A, first half.  A list of four lights and records that name all four, so that every candidate's v is a recorded one: with every
    v above the floor, doubling all of them -- an exact scaling of every u_i and of U in fp32 -- leaves the chosen lights, f and both images
    bit for bit; equal values (8, 16 or 32 for all) give the list's own picks, f and images; below the floor the values stop counting: 1, 2
    and 3 for all are 4 for all.  The first frame has no valid history; the comparison is on frames 1 and 2, where every covered pixel has."""
    lights = four_lights()
    e = LV.entry
    rec = lambda vs: [e(v, k) for k, v in enumerate(vs)]
    plain = picks(lights, None)
    uneven, doubled = picks(lights, rec((5, 10, 20, 7))), picks(lights, rec((10, 20, 40, 14)))
    differs = 0
    for f in (1, 2):
        assert uneven[f]["valid"] and doubled[f]["valid"]
        for k in ("refl", "diff", "chosen", "f", "terms"):
            assert np.array_equal(uneven[f][k], doubled[f][k]), (f, k)
        differs += int((uneven[f]["chosen"] != plain[f]["chosen"]).sum())
    assert differs > 20      # (the uneven values do move the pick)
    for vs in ((8,) * 4, (16,) * 4, (32,) * 4, (1, 2, 3, 4), (4,) * 4):
        even = picks(lights, rec(vs))
        for f in (1, 2):
            for k in ("refl", "diff", "chosen", "f", "terms"):
                assert np.array_equal(even[f][k], plain[f][k]), (vs, f, k)
    assert (plain[1]["chosen"] != LL.NONE).sum() > 1000 and len(set(plain[1]["chosen"][plain[1]["chosen"] != LL.NONE].tolist())) >= 3


def test_with_all_records_free_the_images_are_the_lists_own():
    """Test A, second half: the golden list, every record free in front of every frame -- v_i = 63 for every light.  u_i = w_i 63 is not an
    exact scaling in fp32, so U / u_i and W / w_i may differ in their last bit; what is asserted is what the feature promises to a caller:
    both packed images, bit for bit, and the same chosen lights, on these frames."""
    free = [LV.FREE] * 4
    plain, got = picks(LIGHTS, None, frames=4), picks(LIGHTS, free, frames=4)
    for f in range(4):
        assert np.array_equal(got[f]["chosen"], plain[f]["chosen"]), f
        assert np.array_equal(got[f]["refl"], plain[f]["refl"]) and np.array_equal(got[f]["diff"], plain[f]["diff"]), f
        rel = np.abs(got[f]["f"] - plain[f]["f"]) / np.maximum(plain[f]["f"], 1e-30)
        assert rel.max() <= 2.0 ** -21, (f, rel.max())      # (a few roundings of 2^-24 each)
    assert (plain[0]["chosen"] != LL.NONE).sum() > 2000


# ---- test B: the estimator -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scrambled", [False, True], ids=["the history as it comes", "both record images overwritten with arbitrary bytes"])
def test_the_mean_over_frames_converges_to_the_sum_over_all_lights(scrambled):
    """An unbiased estimator halves its error from 64 to 256 frames; a biased one plateaus (the bar of tests/test_light_list_host.py).  The
    second run overwrites both record images in front of every frame -- valid stamps, random entries: history cannot bias."""
    err, _, _, pixels = run(LIGHTS, 1, 256, scrambled)
    key = "convergence_scrambled" if scrambled else "convergence"
    print("%s: %d pixels, relative L2 %.5f after 64 frames, %.5f after 256, ratio %.3f" % (key, pixels, err[64], err[256], err[256] / err[64]))
    assert pixels > 2000
    assert err[256] / err[64] <= 0.7, err
    assert abs(err[64] - GOLDEN[key]["frames64"]) <= 1e-9 and abs(err[256] - GOLDEN[key]["frames256"]) <= 1e-9, err


# ---- test C: the benefit ---------------------------------------------------------------------------------------------------------------------
def test_it_helps_where_the_brightest_lamps_are_hidden():
    """The standing golden scene at radius 0, frames 16 .. 63: more of the traced shadow rays come back unoccluded than without the records,
    and the error of the mean after 64 frames is below the list's.  No margin beyond "better than the list alone"."""
    got = benefit(LIGHTS)
    print("unoccluded share of the traced shadow rays, frames 16 .. 63: the list %.4f, with the records %.4f; relative L2 after 64 frames: %.5f, %.5f"
          % (got["list_unoccluded_share"], got["unoccluded_share"], got["list_frames64"], got["frames64"]))
    assert got["unoccluded_share"] > got["list_unoccluded_share"], got
    assert got["frames64"] < got["list_frames64"], got
    g = GOLDEN["helps"]
    assert all(abs(got[k] - g[k]) <= 1e-9 for k in g), (got, g)


# ---- the class conditions of the scene and the list the GPU tests use --------------------------------------------------------------------------
def test_the_golden_list_is_the_generators():
    assert LIGHTS == golden_lights(GOLDEN["seed"]) and len(LIGHTS) == 73 >= 65 and GOLDEN["camera"] == CAMERA
    assert {k: GOLDEN[k] for k in ("width", "height", "metallic")} == {k: LIST[k] for k in ("width", "height", "metallic")}
    assert sum(1 for l in LIGHTS[64:] if min(l["intensity"]) >= 300.0) >= 6      # the bright lamps, all in the second chunk


def test_the_class_conditions_of_a_camera_that_stands_moves_and_jumps():
    """Every figure the golden file records is a condition met, on the restatement alone, with a count above zero."""
    frames = class_frames(LIGHTS)
    c = GOLDEN["camera"]
    print("classes: %s" % LV.total(frames))
    LV.check_conditions(frames, "golden")
    assert frames[0]["valid"] == 0 and frames[0]["sequence"] > 0 and frames[1]["valid"] > 0 and all(fr["sequence"] == 0 for fr in frames[1:])
    assert frames[-1]["off_frame"] > 0 and sum(fr["off_frame"] for fr in frames[:c["still"]]) == 0
    assert sum(fr["evicted"] for fr in frames[:12]) > 0 and sum(fr["hidden_from_64"] for fr in frames[:12]) > 0      # (what the GPU tests' twelve frames can hold)
    assert LV.total(frames) == GOLDEN["classes"], LV.total(frames)
    assert frames == GOLDEN["class_frames"]
