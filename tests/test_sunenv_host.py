"""The sun from the environment, the part that needs no GPU: rtggx_sun_from_env declared, exported and bound; the -sunfromenv flag refused at
parse time; the identities of the restatement (tests/sunenv_ref.py) on the synthetic cubes (tests/sunenv_cases.py); and the host's
arithmetic (raytracedggx_amd/csrc/rt_sun_env.h), which includes nothing of HIP: tests/sun_env_main.cpp -- a program of its own -- is built
with a host compiler under AddressSanitizer and UBSan and run as a child process.  The runtimes are linked into the program
(-static-libasan): nothing is preloaded and nothing is loaded into Python."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import host_support as HS
import sunenv_cases as SC
import sunenv_ref as SR

CSRC = os.path.join(HS.ROOT, "raytracedggx_amd", "csrc")
SIGNATURE = (r"\bint\s+rtggx_sun_from_env\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*float\s+cone_degrees\s*,\s*float\s+ring_degrees\s*,\s*float\s+min_contrast\s*,"
             r"\s*int\s+remove\s*,\s*RtggxSunEstimate\s*\*\s*out\s*\)")


def test_the_entry_point_is_declared_exported_and_bound(built):
    HS.declared_exported_bound("rtggx_sun_from_env", SIGNATURE, defines=(r"\bRTGGX_BUF_COUNT\s*=\s*28\b", r"typedef\s+struct\s+RtggxSunEstimate\b", r"224 bytes"))
    from raytracedggx_amd import capi
    import ctypes as C
    assert C.sizeof(capi.SunEstimate) == 224 and capi.SunEstimate.background_half.offset == 19 * 8 and capi.SunEstimate.found.offset == 19 * 8 + 9 * 4


def test_the_executable_refuses_a_bad_flag_before_asking_for_a_device(built):
    sun = ["-sun", "0", "1", "0", "1", "1", "1"]
    HS.executable_refuses([["-sunfromenv", "0"], ["-sunfromenv", "45.5"], ["-sunfromenv", "-3"], ["-sunfromenv", "nan"], ["-sunfromenv", "wide"], ["-sunfromenv", "4x"],
                           ["-sunfromenv"] + sun, sun + ["-sunfromenv", "20"], ["-sunfromenv", "-rayrate", "4"], ["-rayrate", "4", "-sunfromenv", "10"]],
                          must_mention="-sunfromenv")
    # -sunreflections goes with either sun, and without one it is refused with the words it always had
    HS.executable_refuses([["-sunreflections"]], must_mention="-sunreflections without -sun: there is no light to reflect")


# ---- the model's identities ----------------------------------------------------------------------------------------------------------------
CASES = SC.gpu_cases()


@pytest.fixture(scope="module")
def records():
    return {c.name: SR.estimate(c.codes, **c.args) for c in CASES}


def test_the_cases_are_what_they_were_built_to_be(records):
    """The peak where it was put, the cone on as many faces as the place says; at S = 16 and 37 the counts of cone and ring texels the mask
    rule gives at 20 / 40 degrees (a change of the rule, or of the cases, shows here first)."""
    counts = {(16, "centre"): (25, 121), (16, "edge"): (50, 136), (16, "corner"): (68, 125), (37, "centre"): (145, 604), (37, "edge"): (272, 726), (37, "corner"): (372, 657)}
    for c in CASES:
        r = records[c.name]
        if c.peak is not None:
            assert (r["peak_face"], r["peak_x"], r["peak_y"]) == c.peak, c.name
        if c.faces is not None:
            assert len(set((np.nonzero(r["cone_mask"])[0] // (c.S * c.S)).tolist())) == c.faces, c.name
        m = re.match(r"S(16|37)_face\d_(\w+)$", c.name)
        if m:
            assert (r["texels_cone"], r["texels_ring"]) == counts[(int(m.group(1)), m.group(2))], c.name
            assert r["found"] == 1 and r["texels_cone"] >= 20 and r["texels_ring"] >= 100 and r["texels_lit"] >= 20, c.name
    # S = 64 with the default angles (4 / 12 degrees): what the same rule gives at the face centre and in the corner
    assert (records["S64_face5_centre"]["texels_cone"], records["S64_face5_centre"]["texels_ring"]) == (19, 126)
    assert (records["S64_face5_corner"]["texels_cone"], records["S64_face5_corner"]["texels_ring"]) == (69, 416)


def test_original_equals_residual_plus_excess_exactly(records):
    """Per texel and channel, on the sanitised values; and the cut level 0 holds the residual in the cone and the original's bits elsewhere."""
    for c in CASES:
        r = records[c.name]
        residual, e = SR.split(c.codes, r)
        assert np.array_equal(residual + e, SR.values(c.codes)), c.name
        assert (e[~r["cone_mask"]] == 0).all() and (residual[r["cone_mask"]] <= r["background_half"].astype(np.float64)).all(), c.name
        cut = SR.removed_level0(c.codes, r)
        assert np.array_equal(cut.reshape(-1, 4)[~r["cone_mask"]], c.codes.reshape(-1, 4)[~r["cone_mask"]]), c.name
        assert np.array_equal(SR.values(cut)[r["cone_mask"]], residual[r["cone_mask"]]) and np.array_equal(cut[..., 3], c.codes[..., 3]), c.name


def test_a_constant_cube_plus_a_sun_gives_the_constant_back_and_the_suns_weighted_sum():
    """c0 a binary16 value everywhere, plus s on a set of cone texels (every c0 + s a binary16 value as well): b16 == c0, and excess == sum w s
    to the summation bound."""
    S, c0, s = 16, 0.5, np.array([512.0, 384.0, 256.0])
    rgb = np.full((6 * S * S, 3), c0)
    peak = (4 * S + 9) * S + 7
    lit = [peak, peak + 1, peak - S, peak + S + 1]
    rgb[lit] += s * np.array([1.0, 0.5, 0.25, 0.125])[:, None]
    r = SR.estimate(SC.codes_of(S, rgb), 20.0, 40.0)
    assert r["found"] == 1 and (r["background_half"] == np.float32(c0)).all() and r["cone_mask"][lit].all() and r["texels_lit"] == 4
    D = SR.directions(S).astype(np.float64)
    n = (D * D).sum(axis=1)
    w = (4.0 * S) / (n * np.sqrt(n))
    for ch in range(3):
        terms = [float(w[i]) * float(s[ch]) * k for i, k in zip(lit, (1.0, 0.5, 0.25, 0.125))]
        assert abs(r["excess"][ch] - math.fsum(terms)) <= SR.DERIVED_BOUND * math.fsum(terms), ch


def test_the_six_faces_give_the_same_sums_up_to_the_summation_bound():
    """The same sun at the centre of each face over a constant background: only the order of the terms changes."""
    recs = []
    for face in range(6):
        codes, _ = SC.sun_cube(16, face, "centre", 12.0, smooth=False, seed=-17 * face)      # (sun_cube adds 17 face to the seed: one background for all)
        recs.append(SR.estimate(codes, 20.0, 40.0))
    first = recs[0]
    for r in recs[1:]:
        assert (r["texels_cone"], r["texels_ring"], r["texels_lit"], r["peak_luma"]) == (first["texels_cone"], first["texels_ring"], first["texels_lit"], first["peak_luma"])
        assert (r["background_half"] == first["background_half"]).all()
        for k in ("weight_all", "weight_cone", "weight_ring", "ring_rgb", "excess"):
            assert np.all(np.abs(np.asarray(r[k]) - np.asarray(first[k])) <= 2.0 * SR.DERIVED_BOUND * np.asarray(first["magnitude"][k])), k
        assert abs(np.linalg.norm(r["moment"]) - np.linalg.norm(first["moment"])) <= 2.0 * SR.DERIVED_BOUND * first["magnitude"]["moment"].sum()


def test_no_sun_on_the_constant_and_the_black_cube(records):
    for name in ("constant", "black"):
        r = records[name]
        assert r["found"] == 0 and r["removed"] == 0 and r["texels_lit"] == 0 and not r["direction"].any() and not r["irradiance"].any(), name
    assert records["black"]["peak_luma"] == 0.0 and records["constant"]["peak_luma"] == records["constant"]["mean_luma"] == 0.75


def test_the_plateau_goes_to_the_lowest_index_and_the_hostile_texels_count_as_the_rule_says(records):
    assert (records["plateau"]["peak_face"], records["plateau"]["peak_x"], records["plateau"]["peak_y"]) == (1, 3, 2)
    h = records["hostile"]
    case = [c for c in CASES if c.name == "hostile"][0]
    raw = case.codes[..., :3].view(np.float16).astype(np.float64).reshape(-1, 3)
    assert np.isnan(raw[h["cone_mask"]]).any() and (raw[h["cone_mask"]] < 0).any() and np.isnan(raw[h["ring_mask"]]).any()
    assert h["peak_luma"] == (0.25 * 65504.0 + 0.5 * 65504.0) + 0.25 * 8192.0 and h["found"] == 1 and np.isfinite(h["irradiance"]).all()
    assert np.isfinite(SR.values(SR.removed_level0(case.codes, h))[h["cone_mask"]]).all()


# ---- the host's arithmetic, stand-alone under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to build the stand-alone program with")
    exe = str(tmp_path_factory.mktemp("sun_env") / "sun_env")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-o", exe, os.path.join(HS.ROOT, "tests", "sun_env_main.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b|unrecognized (command[- ]line )?option .*-fsanitize", r.stderr):
        pytest.skip("the sanitizer runtime is missing: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    return exe


def clean(r):
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr)
    return r.stdout


def test_the_host_arithmetic_under_address_and_undefined_behaviour_sanitizers(program):
    """Defaults and refusals of the arguments, the cosines, the integer directions, every binary16 rounding case, the background and its
    cap, the found decision at its edge, direction and irradiance and their refusals.  The program must end clean."""
    assert re.search(r"sun env: all \d+ checks passed", clean(subprocess.run([program], capture_output=True, text=True, timeout=120)))


def test_the_host_arithmetic_equals_the_restatement_bit_for_bit(program, records):
    """The sums of the model's records handed to the header's functions: background, its half, the mean, found, direction and irradiance."""
    for c in CASES:
        r = records[c.name]
        nums = list(r["ring_rgb"]) + [r["weight_ring"], r["peak_luma"], r["sum_wy"], r["weight_all"]] + list(r["moment"]) + list(r["excess"])
        out = clean(subprocess.run([program, "record"] + [float(x).hex() for x in nums] + [repr(float(SR.angles(**c.args)[2]))], capture_output=True, text=True, timeout=60))
        line = dict(l.split(" ", 1) for l in out.strip().splitlines())
        assert [int(x, 16) for x in line["background"].split()] == [int(np.float64(x).view(np.uint64)) for x in r["background"]], c.name
        assert [int(x, 16) for x in line["half"].split()] == [int(x) for x in r["b16_codes"]], c.name
        assert [int(x, 16) for x in line["half_as_float"].split()] == [int(x) for x in r["background_half"].view(np.uint32)], c.name
        mean, found, result = re.match(r"(\w+) found (\d) result (\d)", line["mean"]).groups()
        assert int(mean, 16) == int(np.float64(r["mean_luma"]).view(np.uint64)), c.name
        assert (int(found) and int(result)) == r["found"], c.name      # (a record that stopped before pass C holds a zero moment: no result either)
        if r["found"]:
            assert [int(x, 16) for x in line["direction"].split()] == [int(x) for x in r["direction"].view(np.uint32)], c.name
            assert [int(x, 16) for x in line["irradiance"].split()] == [int(x) for x in r["irradiance"].view(np.uint32)], c.name


def test_the_header_includes_nothing_of_hip():
    with open(os.path.join(CSRC, "rt_sun_env.h")) as f:
        header = f.read()
    assert sorted(re.findall(r"^\s*#\s*include\s*(\S+)", header, re.M)) == ["<cmath>", "<cstdint>", "<cstring>"]
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__shared__", header)
