"""Light lists that move, the part that needs no GPU: the five entry points declared, exported and bound; -lightlistorbit checked at parse
time; the check and conversion of one light (raytracedggx_amd/csrc/rt_light_check.h, which the host and lightListPrepareKernel share) run
in a program of its own (tests/light_prepare_main.cpp), plain and under AddressSanitizer and UBSan, against numpy in float64 rounded once;
and the restatement (tests/light_list_moving_ref.py) over the eight frames of the motion the GPU tests use, with the conditions that keep
those tests from being vacuous (tests/golden/light_list_moving_classes.json).

    python tests/test_light_list_moving_host.py --write-golden

writes tests/golden/light_list_moving_classes.json: the figures the restatement gives for the motion."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import host_support as HS
import light_list_moving_ref as LM
import light_list_ref as LL
import light_list_vis_ref as LV

GOLDEN_PATH = os.path.join(HS.ROOT, "tests", "golden", "light_list_moving_classes.json")
SCENE = json.load(open(os.path.join(HS.ROOT, "tests", "golden", "light_list_vis_classes.json")))      # 148 x 84, mixed materials, 73 lights, lamps 64 .. 72 behind the model
W, H, MIXED, LIGHTS = SCENE["width"], SCENE["height"], tuple(SCENE["metallic"]), SCENE["lights"]
EYE, STEP, DT = (10.0, 10.0, -24.0), (0.3, 0.1, 0.2), 0.25      # the camera of the restatement's run: a small step a frame, so that reprojected taps stay valid


def eye(f):
    return tuple(EYE[k] + STEP[k] * f for k in range(3))


def moving_run(reset_every_frame=False):
    """The eight frames under the moving camera, records on: per frame the class counts, the kept counts and the chosen light per pixel.
    reset_every_frame: the history reset in front of every frame -- what rtggx_set_light_list per frame, the only way before, does."""
    rows = LL.records(LIGHTS)
    o = LM.Oracle(W, H)
    try:
        HS.scene(o, metallic=MIXED)
        o.set_light_list(LIGHTS); o.set_light_list_visibility(1)
        out = []
        for f in range(LM.FRAMES):
            o.update_light_list(LM.motion(rows, f))
            if reset_every_frame:
                o.seq0 = o.seq
            o.camera_frame(eye(f), DT)
            assert o.acted and o.seq == f + 1
            out.append(dict(counts=LV.counts(o), kept=o.list_kept.copy(), chosen=o.list_info[..., 1].copy()))
        return out
    finally:
        o.close()


def figures():
    kept, reset = moving_run(), moving_run(reset_every_frame=True)
    return dict(frames=[r["counts"] for r in kept], total=LV.total([r["counts"] for r in kept]),
                blocks_whose_kept_count_differs_first_to_last=int((kept[0]["kept"] != kept[-1]["kept"]).sum()),
                pixel_frames_picked_differently_with_the_history_kept=int(sum((a["chosen"] != b["chosen"]).sum() for a, b in zip(kept, reset))))


def check_conditions(g):
    """The issue's conditions: valid history in every frame after the first; lit, occluded and inserted above 0; the kept counts of the first
    and the last frame differ; a pixel-frame picks another light than the run whose history is reset every frame."""
    assert g["frames"][0]["valid"] == 0 and all(f["valid"] > 0 for f in g["frames"][1:]), [f["valid"] for f in g["frames"]]
    for k in ("lit", "occluded", "inserted"):
        assert g["total"][k] > 0, (k, g["total"])
    assert g["blocks_whose_kept_count_differs_first_to_last"] > 0
    assert g["pixel_frames_picked_differently_with_the_history_kept"] > 0


def write_golden():
    g = figures()
    check_conditions(g)
    out = dict(width=W, height=H, frames_of_motion=LM.FRAMES, degrees_per_frame=LM.DEGREES, travel=list(LM.TRAVEL), eye=list(EYE), step=list(STEP), dt=DT, **g)
    with open(GOLDEN_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in out if k != "frames"}, indent=1))


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-golden"]:
        write_golden()
    sys.exit(0)


# ---- declared, exported, bound ---------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound(built):
    ctx = r"rtggx_context\s*\*\s*ctx"
    HS.declared_exported_bound(
        "rtggx_update_light_list", r"\bint\s+rtggx_update_light_list\s*\(\s*" + ctx + r"\s*,\s*const\s+RtggxLight\s*\*\s*lights\s*,\s*uint32_t\s+first\s*,\s*uint32_t\s+count\s*\)",
        defines=(r"#define\s+RTGGX_LIGHT_KIND_RADIUS\s+1u", r"#define\s+RTGGX_LIGHT_KIND_CONE\s+2u", r"s0 stays", r"PRESUMED CASTING", r"The number of lights never changes",
                 r"Calls apply in call order", r"ordered like hipMemcpyAsync on hip_stream", r"A frame without an update launches and copies nothing", r"the count is fixed"),
        method="update_light_list")
    HS.declared_exported_bound(
        "rtggx_update_light_list_device",
        r"\bint\s+rtggx_update_light_list_device\s*\(\s*" + ctx + r"\s*,\s*const\s+RtggxLight\s*\*\s*device_lights\s*,\s*uint32_t\s+first\s*,\s*uint32_t\s+count\s*,\s*uint32_t\s+kinds\s*,\s*void\s*\*\s*hip_stream\s*\)",
        method="update_light_list_device")
    HS.declared_exported_bound("rtggx_read_light_list", r"\bint\s+rtggx_read_light_list\s*\(\s*" + ctx + r"\s*,\s*RtggxLight\s*\*\s*out\s*,\s*size_t\s+bytes\s*\)", method="read_light_list")
    HS.declared_exported_bound("rtggx_read_light_list_rejects", r"\bint\s+rtggx_read_light_list_rejects\s*\(\s*" + ctx + r"\s*,\s*uint64_t\s*\*\s*rejects\s*,\s*int\s+reset\s*\)",
                               method="read_light_list_rejects")
    HS.declared_exported_bound("rtggx_debug_visibility_drains", r"\bint\s+rtggx_debug_visibility_drains\s*\(\s*" + ctx + r"\s*,\s*uint32_t\s*\*\s*drains\s*,\s*int\s+reset\s*\)",
                               method="debug_visibility_drains")
    from raytracedggx_amd import app, capi
    L = capi.load()
    assert L.rtggx_update_light_list.argtypes == [C.c_void_p, C.POINTER(capi.Light), C.c_uint32, C.c_uint32]
    assert L.rtggx_update_light_list_device.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    assert (capi.LIGHT_KIND_RADIUS, capi.LIGHT_KIND_CONE) == (1, 2) == (LM.KIND_RADIUS, LM.KIND_CONE)
    host = C.CDLL(app.HOST_LIB_PATH)
    for name in ("rtggx_app_update_light_list", "rtggx_app_update_light_list_device", "rtggx_app_read_light_list"):
        assert name in app.HOST_EXPORTS and hasattr(host, name)
    for name in ("update_light_list", "update_light_list_device", "read_light_list"):
        assert callable(getattr(app.RayTracedGGX, name, None))
    for name in ("RayTracedGGX.h", "RayTracedGGX.cpp"):      # the flag list and kFlags
        text = open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", name)).read()
        assert "-lightlistorbit" in text and ('"lightlistorbit"' in text or name.endswith(".h"))
    header = open(os.path.join(HS.ROOT, "raytracedggx_amd", "host", "RayTracer.h")).read()
    assert all(n in header for n in ("UpdateLightList", "UpdateLightListDevice", "ReadLightList"))
    assert "lights that move need a new" not in open(os.path.join(HS.ROOT, "include", "rtggx.h")).read()


def list_file(tmp_path, lights):
    lines = ["light " + " ".join(repr(float(x)) for x in list(l["position"]) + list(l["intensity"]) + [l["range"]] + ([l["radius"]] if "radius" in l else [])) for l in lights]
    path = tmp_path / "lights.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_the_executable_refuses_the_orbit_without_a_list_and_parses_it_with_one(built, tmp_path):
    import assets
    good, missing = list_file(tmp_path, LIGHTS), str(tmp_path / "missing.hdr")
    HS.executable_refuses([(["-lightlistorbit", "3"], "-lightlistorbit without -lightlist"),
                           (["-lightlistorbit", "3", "-light", "1", "2", "3", "4", "5", "6", "7"], "-lightlistorbit without -lightlist"),
                           (["-lightlist", good, "-lightlistorbit", "fast"], "-lightlistorbit: fast"),
                           (["-lightlist", good, "-lightlistorbit"], "-lightlistorbit: degrees per frame")])
    # what stops these runs is the environment file, which is read after the command line and before a device is asked for
    HS.executable_refuses([["-env", missing, "-lightlist", good, "-lightlistorbit", "3"], ["-env", missing, "-lightlistorbit", "-2.5", "-lightlist", good, "-lightlistvisibility"]],
                          must_mention="cannot open", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


# ---- the shared check and conversion, in a program of its own ---------------------------------------------------------------------------------
def light(position=(1.0, 2.0, 3.0), range_=10.0, intensity=(5.0, 6.0, 7.0), radius=0.0, axis=(0.0, 0.0, 0.0), cos_outer=-1.0, cos_inner=1.0, pad=(9.0, 9.0, 9.0)):
    f = np.zeros(16, np.float32)
    f[0:3], f[3], f[4:7], f[7], f[8:11], f[11], f[12], f[13:16] = position, range_, intensity, radius, axis, cos_outer, cos_inner, pad
    return f


NAN, INF = float("nan"), float("inf")
SUB = float(np.float32(1e-42))      # a subnormal fp32
# (the light, the kinds declared, the reason): every refusal reason, and the edges the issue names
TABLE = [
    (light(), 3, LM.OK), (light(), 0, LM.OK),
    (light(position=(NAN, 0, 0)), 3, LM.BAD_POSITION), (light(position=(0, INF, 0)), 3, LM.BAD_POSITION | 1 << 8), (light(position=(0, 0, -INF)), 3, LM.BAD_POSITION | 2 << 8),
    (light(range_=0.0), 3, LM.BAD_RANGE), (light(range_=-1.0), 3, LM.BAD_RANGE), (light(range_=INF), 3, LM.BAD_RANGE), (light(range_=NAN), 3, LM.BAD_RANGE),
    (light(intensity=(-1.0, 0, 0)), 3, LM.BAD_INTENSITY), (light(intensity=(0, NAN, 0)), 3, LM.BAD_INTENSITY | 1 << 8), (light(intensity=(0, 0, INF)), 3, LM.BAD_INTENSITY | 2 << 8),
    (light(intensity=(-0.0, -0.0, -0.0)), 3, LM.OK),      # -0.0: accepted, casts nothing
    (light(intensity=(0.0, 0.0, 0.0)), 3, LM.OK), (light(intensity=(0.0, SUB, 0.0)), 3, LM.OK),
    (light(radius=-0.5), 3, LM.BAD_RADIUS), (light(radius=NAN), 3, LM.BAD_RADIUS), (light(radius=10.0), 3, LM.BAD_RADIUS),      # a radius equal to the range
    (light(radius=11.0), 3, LM.BAD_RADIUS), (light(radius=float(np.nextafter(np.float32(10.0), np.float32(0.0)))), 3, LM.OK),
    (light(radius=1.0), 3, LM.OK), (light(radius=1.0), LM.KIND_CONE, LM.UNDECLARED_RADIUS), (light(radius=1.0), 0, LM.UNDECLARED_RADIUS), (light(radius=1.0), LM.KIND_RADIUS, LM.OK),
    (light(axis=(0, 0, 0), cos_outer=0.5), 3, LM.BAD_AXIS), (light(axis=(NAN, 1, 0), cos_outer=0.5), 3, LM.BAD_AXIS), (light(axis=(INF, 1, 0), cos_outer=0.5), 3, LM.BAD_AXIS),
    (light(axis=(0, 0, 1), cos_outer=0.5, cos_inner=0.5), 3, LM.BAD_COSINES), (light(axis=(0, 0, 1), cos_outer=0.5, cos_inner=1.5), 3, LM.BAD_COSINES),
    (light(axis=(0, 0, 1), cos_outer=0.5, cos_inner=NAN), 3, LM.BAD_COSINES), (light(axis=(0, 0, 1), cos_outer=0.9, cos_inner=0.8), 3, LM.BAD_COSINES),
    (light(cos_outer=NAN), 3, LM.BAD_COS_OUTER), (light(cos_outer=NAN, axis=(0, 0, 1)), 0, LM.BAD_COS_OUTER),
    (light(cos_outer=-1.0, axis=(NAN, NAN, NAN)), 3, LM.OK), (light(cos_outer=-INF), 3, LM.OK), (light(cos_outer=-5.0, cos_inner=NAN), 0, LM.OK),      # no cone: axis and inner not read
    (light(axis=(0, 0, 1), cos_outer=0.5, cos_inner=0.75), 3, LM.OK), (light(axis=(0, 0, 1), cos_outer=0.5, cos_inner=0.75), LM.KIND_RADIUS, LM.UNDECLARED_CONE),
    (light(axis=(0, 0, 1), cos_outer=0.5, cos_inner=0.75), 0, LM.UNDECLARED_CONE), (light(axis=(0, 0, 1), cos_outer=0.5, cos_inner=0.75, radius=2.0), LM.KIND_CONE, LM.UNDECLARED_RADIUS),
    (light(axis=(SUB, 0, 0), cos_outer=0.5), 3, LM.OK), (light(axis=(SUB, -SUB, 3 * SUB), cos_outer=0.0, cos_inner=1.0), 3, LM.OK),      # subnormal axes: the squares are exact in double
    (light(axis=(3e38, -3e38, 1e38), cos_outer=-0.5, cos_inner=0.25), 3, LM.OK), (light(axis=(3.4e38, 3.4e38, 3.4e38), cos_outer=0.5), 3, LM.OK),      # huge: no overflow in double
    (light(axis=(1.0, 2.0, -3.0), cos_outer=0.1, cos_inner=0.2), 3, LM.OK), (light(axis=(0.3, 0.4, 0.5), cos_outer=-0.999, cos_inner=1.0, radius=0.25), 3, LM.OK),
    (light(axis=(1e-3, 7.0, 1e3), cos_outer=0.5, intensity=(0, 0, 0)), 3, LM.OK),
]


def run_program(exe, tmp_path):
    src, dst = tmp_path / "lights.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.uint32(len(TABLE)).tobytes())
        for row, kinds, _ in TABLE:
            f.write(np.uint32(kinds).tobytes()); f.write(np.asarray(row, np.float32).tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr)
    out = np.fromfile(dst, np.uint32).reshape(len(TABLE), 37)
    return r.stdout, out[:, 0], out[:, 1:17], out[:, 17:21], out[:, 21:37]


def check_program(exe, tmp_path):
    stdout, reasons, recs, cull, kept = run_program(exe, tmp_path)
    rejects = 0
    for i, (row, kinds, want) in enumerate(TABLE):
        assert LM.check(row, kinds) == want, (i, LM.check(row, kinds), want)      # the numpy restatement agrees with the table
        assert int(reasons[i]) == want, "light %d: reason %d, expected %d" % (i, reasons[i], want)
        if want == LM.OK:
            r, q = LM.convert(row)
            k = np.array(row, np.float32)
            if row[11] > -1:
                k[8:11] = r[8:11]
            np.testing.assert_array_equal(kept[i], k.view(np.uint32), err_msg="light %d: what the context keeps" % i)
        else:
            r, q = LM.sanitised()
            rejects += 1
            assert not kept[i].any()
        np.testing.assert_array_equal(recs[i], r.view(np.uint32), err_msg="light %d: the record" % i)
        np.testing.assert_array_equal(cull[i], q.view(np.uint32), err_msg="light %d: the cull entry" % i)
    assert rejects > 10 and ("light prepare: %d lights, %d rejects" % (len(TABLE), rejects)) in stdout
    minus_zero = next(i for i, (row, _, _) in enumerate(TABLE) if np.signbit(row[4]) and row[4] == 0)
    assert cull[minus_zero].view(np.float32)[3] == 0.0 and recs[minus_zero].view(np.float32)[3] == 10.0      # accepted, never kept
    unit = [np.linalg.norm(recs[i].view(np.float32)[8:11].astype(np.float64)) for i, (row, _, want) in enumerate(TABLE) if want == LM.OK and row[11] > -1]
    assert len(unit) >= 8 and all(abs(u - 1.0) < 2e-7 for u in unit), unit


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "under ASan and UBSan"])
def test_the_shared_check_and_conversion_equal_numpy(tmp_path, sanitized):
    """tests/light_prepare_main.cpp over the table: reason codes, records, cull entries and the kept copies bit for bit what numpy gives in
    float64, rounded once.  The sanitizer runtimes are linked into the program: nothing is preloaded and nothing is loaded into Python."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to build the stand-alone program with")
    exe = str(tmp_path / "light_prepare")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off"]
    if sanitized:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run([gxx] + flags + ["-o", exe, os.path.join(HS.ROOT, "tests", "light_prepare_main.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and sanitized and re.search(r"cannot find -l(asan|ubsan)\b|unrecognized (command[- ]line )?option .*-fsanitize", r.stderr):
        pytest.skip("the sanitizer runtime is missing: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    check_program(exe, tmp_path)


def test_the_header_is_free_of_hip():
    header = open(os.path.join(HS.ROOT, "raytracedggx_amd", "csrc", "rt_light_check.h")).read()
    assert sorted(re.findall(r"^\s*#\s*include\s*(\S+)", header, re.M)) == ["<stdint.h>"]


# ---- the restatement over the motion ----------------------------------------------------------------------------------------------------------
def test_the_motion_is_computed_from_the_originals_and_moves_what_it_says():
    rows = LL.records(LIGHTS)
    first, last = LM.motion(rows, 0), LM.motion(rows, LM.FRAMES - 1)
    np.testing.assert_array_equal(first, rows)
    np.testing.assert_array_equal(last[LM.LAMPS, 0:3], (rows[LM.LAMPS, 0:3].astype(np.float64) + np.array(LM.TRAVEL)).astype(np.float32))
    np.testing.assert_array_equal(last[:, 3:8], rows[:, 3:8])
    lattice = last[:64, 0:3].astype(np.float64)
    np.testing.assert_allclose(np.hypot(lattice[:, 0], lattice[:, 2]), np.hypot(rows[:64, 0].astype(np.float64), rows[:64, 2].astype(np.float64)), rtol=3e-7)
    assert (rows[LM.LAMPS, 2] > 0).all() and (last[LM.LAMPS, 2] < 0).all()      # from behind the model to in front of it
    for f in range(LM.FRAMES):
        assert all(LM.check(r) == LM.OK for r in LM.motion(rows, f))


def test_an_update_keeps_s0_and_a_new_list_does_not():
    o = LM.Oracle(64, 36)
    try:
        o.set_light_list(LIGHTS); o.set_light_list_visibility(1)
        o.seq = 5
        o.update_light_list(LIGHTS[:3], first=2)
        assert o.seq0 == 0
        np.testing.assert_array_equal(o.light_list[2:5], LL.records(LIGHTS[:3]))
        np.testing.assert_array_equal(o.light_list[5:], LL.records(LIGHTS)[5:])
        with pytest.raises(ValueError):
            o.update_light_list(LIGHTS[:2], first=len(LIGHTS) - 1)
        with pytest.raises(ValueError):
            o.update_light_list([dict(LIGHTS[0], range=-1.0)])
        dark = [dict(l, intensity=[0.0, 0.0, 0.0]) for l in LIGHTS]
        o.update_light_list(dark)
        assert not o.acting()
        o.presumed_casting = True
        assert o.acting()
        o.set_light_list(LIGHTS)
        assert o.seq0 == 5 and not o.presumed_casting
    finally:
        o.close()


def test_the_motions_eight_frames_meet_the_conditions_and_the_golden_file():
    """The conditions that keep the GPU tests from being vacuous, and the figures of tests/golden/light_list_moving_classes.json."""
    g = figures()
    print("moving list: %s; kept counts differ in %d blocks; %d pixel-frames pick differently" % (
        g["total"], g["blocks_whose_kept_count_differs_first_to_last"], g["pixel_frames_picked_differently_with_the_history_kept"]))
    check_conditions(g)
    golden = json.load(open(GOLDEN_PATH))
    for k in ("frames", "total", "blocks_whose_kept_count_differs_first_to_last", "pixel_frames_picked_differently_with_the_history_kept"):
        assert g[k] == golden[k], k
