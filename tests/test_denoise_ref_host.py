"""The float64 model of the denoise chain (tests/denoise_ref.py) against the CPU oracle (oracle/orc_denoise.h), per pixel, on the synthetic
inputs of tests/denoise_cases.py.  No GPU.

Two independent statements of the shaders agreeing per pixel validates the model, and the distance between them MEASURES THE FLOOR: what a
faithful fp32 implementation differs from the true value by, in binary16 ulps of the true value (codes for the back buffer).  The floor is
recorded in tests/golden/denoise_synthetic_floor.json and re-measured by every run; tests/test_gpu_denoise_synthetic.py takes its bounds
from it.  Regenerate the file by hand after a deliberate change of the model, the oracle or the cases:

    python -c "import sys; sys.path[:0] = ['tests', '.']; import test_denoise_ref_host as t; t.write_floor()"

(the `gpu_measured` entry, written by the GPU test's own helper, is kept).

For every case and both evaluations of the oracle's normal weight ("exact", "libm"):
  chain           FilteredOut, FilteredOut1 and TemporalSSOut of the model's whole chain against the oracle's (the chained back buffer is
                  counted and recorded, not asserted);
  stage isolated  the model's temporal pass fed the ORACLE's FilteredOut1 words, its tone map fed the oracle's TemporalSSOut words
                  (without the temporal pass's amplification of what came before it: this is the figure the GPU test bounds).
Asserted: the classes finite / infinite / NaN coincide in every channel; the alpha channels (hit flag, history weight) are bit-identical;
back-buffer codes differ only where the model's value is within its stated fp32 bound of a rounding boundary, by one code; ill-conditioned
temporal pixels (denoise_ref.COND_MAX, nowhere else and by no other criterion) lie in the model's interval, and are at most 5 % of the
pixels whose history takes part -- except in the one flat case, which is ill-conditioned by construction; every case shows the facts it
was built for (Case.expect); the measured table reproduces the recorded one.
"""
import json
import os

import numpy as np
import pytest

import denoise_cases as DC
import denoise_ref as R
from oracle import oracle as O

FLOOR_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoise_synthetic_floor.json")
VARIANTS = ("exact", "libm")
ILL_SHARE_CAP = 0.05
# An ill-conditioned pixel's fp32 result is asked to lie in the model's interval, widened by what the comparison itself costs: the
# store's rounding (half an ulp) and the well-conditioned arithmetic around sigma (the floor of the well-conditioned pixels: below 2).
INTERVAL_SLACK_ULPS = 2.0
# The libm variant's figures depend on the host's C library through std::pow in fp32: the recorded figure may move by this much.  The exact
# variant is compared exactly.  It is not free of the C library either -- the Gaussian and the depth weight are fp32 std::exp in both variants
# (orc_denoise.h depth_weight, gaussian) -- so on a host whose expf rounds an argument the other way an exact figure can move, and "the floor
# moved" then means that: re-measure with write_floor() on that host and look at what changed before accepting it.
LIBM_DRIFT_ULPS = 0.25


def run_oracle(case, variant):
    """The oracle's chain on a case -> words of FilteredOut, FilteredOut1, TemporalSSOut, the back buffer."""
    b = DC.check(case)
    o = O.Oracle(case.W, case.H, threads=4)
    try:
        o.set_normal_weight(variant)
        assert o.parity() == 0      # orc_denoise flips first: scratch = TSS1, history = TSS0
        _load_oracle(o, b)
        o.denoise(); o.tone_map()
        out = {"flt_rfl": o.buffer(O.BUF_FLT_RFL), "flt_dff": o.buffer(O.BUF_FLT_DFF), "tss": o.buffer(O.BUF_TSS0 + o.parity()),
               "bb": o.buffer(O.BUF_BACKBUFFER)}
    finally:
        o.set_normal_weight("exact")
        o.close()
    return b, out


def compare_f16(label, got_words, model_value, where=None, pixel_scale=False):
    """Classes and alpha identical (asserted); returns the ulp errors of the pixels in `where` (all by default)."""
    got = R.from_f16_words(got_words)
    np.testing.assert_array_equal(R.classes(got[..., :3]), R.classes(R.from_f16_words(R.to_f16_words(model_value))[..., :3]),
                                  err_msg="%s: finite / infinite / NaN pattern" % label)
    np.testing.assert_array_equal(got_words >> np.uint64(48), R.to_f16_words(model_value) >> np.uint64(48), err_msg="%s: alpha" % label)
    e = R.ulp_error(got_words, model_value, pixel_scale)
    return e if where is None else np.where(where, e, -1.0)


def check_interval(label, got_words, t, slack=INTERVAL_SLACK_ULPS):
    """The ill-conditioned pixels of a temporal result inside the model's interval."""
    got = R.from_f16_words(got_words)[..., :3]
    ill = t["ill"][..., None] & np.isfinite(got) & np.isfinite(t["lo"]) & np.isfinite(t["hi"])
    lo, hi = t["lo"] - slack * R.ulp16(t["lo"]), t["hi"] + slack * R.ulp16(t["hi"])
    bad = ill & ((got < lo) | (got > hi))
    assert not bad.any(), "%s: %d ill-conditioned values outside the model's interval, e.g. %s" % (
        label, int(bad.sum()), [(tuple(i), float(got[tuple(i)]), float(t["lo"][tuple(i)]), float(t["hi"][tuple(i)])) for i in np.argwhere(bad)[:3]])


def compare_backbuffer(label, got_words, x, near):
    """Codes equal to floor(x) except within the fp32 bound of a boundary (denoise_ref.TONEMAP_TIE_CODES), never by more than one code.
    Returns (differing values, near-tie values)."""
    got = O.unpack_rgba8(got_words).astype(np.int64)
    want = np.floor(x).astype(np.int64)
    d = got - want
    assert np.abs(d).max(initial=0) <= 1, "%s: a back-buffer code is off by %d" % (label, int(np.abs(d).max()))
    assert not ((d != 0) & ~near).any(), "%s: %d back-buffer codes differ away from a rounding boundary" % (label, int(((d != 0) & ~near).sum()))
    return int((d != 0).sum()), int(near.sum())


def case_facts(case, m):
    """The facts a case was built for, from the model's outputs (all integers or exact shares)."""
    t = m["temporal"]
    surf = m["surf"]
    long_n = int(t["long"].sum())
    f = {"surface": int(surf.sum()), "holes": int((~surf).sum()), "radii": int(np.unique(m["blur_radius"][surf]).size) if surf.any() else 0,
         "radius_max": int(m["blur_radius"][surf].max()) if surf.any() else 0,
         "nan_flt_rfl": int(np.isnan(m["flt_rfl"][..., :3]).any(-1).sum()), "nonfinite_flt": int((~np.isfinite(m["flt_dff"][..., :3])).any(-1).sum()),
         "wsum_diff_zero": int(((m["wsum_diff"] == 0.0) & m["diffuse"]).sum()), "diffuse": int(m["diffuse"].sum()),
         "long": long_n, "plain": int((~t["long"]).sum()), "ill": int(t["ill"].sum()),
         "over_each_border": int(t["over"].reshape(-1, 4).sum(0).min()), "vmax_moved": int(t["vmax_moved"].sum()), "vmax_ties": int(t["vmax_ties"].sum()),
         "gamma_at_clamp": int(t["gamma_at_clamp"].sum())}
    # surface pixels of a named region whose FilteredOut, FilteredOut1 AND temporal result are finite: values there are compared, not patterns
    fin = surf & np.isfinite(m["flt_rfl"][..., :3]).all(-1) & np.isfinite(m["flt_dff"][..., :3]).all(-1) & np.isfinite(t["value"][..., :3]).all(-1)
    for region, mask in case.regions.items():
        f["finite_" + region] = int((fin & mask).sum())
    return f


def check_expectations(case, f):
    e = case.expect
    for region in case.regions:
        key = "finite_%s_min" % region
        assert f["finite_" + region] >= e[key], "%s went vacuous: %d finite pixels in its %s block, built for at least %d" % (
            case.name, f["finite_" + region], region, e[key])
    for key, name in (("surface_min", "surface"), ("radii_min", "radii"), ("holes_min", "holes"), ("nan_flt_rfl_min", "nan_flt_rfl"),
                      ("wsum_diff_zero_min", "wsum_diff_zero"), ("nonfinite_flt_min", "nonfinite_flt"), ("plain_min", "plain"), ("long_min", "long"),
                      ("over_each_border_min", "over_each_border"), ("vmax_moved_min", "vmax_moved"), ("vmax_ties_min", "vmax_ties"),
                      ("gamma_at_clamp_min", "gamma_at_clamp")):
        if key in e:
            assert f[name] >= e[key], "%s went vacuous: %s = %d, built for at least %d" % (case.name, name, f[name], e[key])
    if "radius_max" in e:
        assert f["radius_max"] == e["radius_max"], "%s: largest blur radius %d, built for %d" % (case.name, f["radius_max"], e["radius_max"])
    if "ill_share_min" in e:
        assert f["ill"] >= e["ill_share_min"] * f["long"]
    if "depth_zero" in e:
        assert (case.depth == 0).any() and (case.depth == 0xFFFFFF).any()
    if not case.flat:
        assert f["ill"] <= ILL_SHARE_CAP * max(f["long"], 1), "%s: %d of %d long-path pixels are ill-conditioned: change the input, not the cap" % (
            case.name, f["ill"], f["long"])


def _load_oracle(o, b):
    for bid, key in ((O.BUF_NORMAL, "normal"), (O.BUF_ROUGH_METAL, "rough_metal"), (O.BUF_DEPTH, "depth"), (O.BUF_VELOCITY, "velocity"),
                     (O.BUF_RT_REFL, "rt_refl"), (O.BUF_RT_DIFF, "rt_diff"), (O.BUF_TSS0, "history"), (O.BUF_TSS1, "scratch")):
        o.buffer(bid, copy=False)[...] = b[key]


@pytest.mark.parametrize("name", ["size_97x61", "normals_97x61", "history_97x61"])
def test_single_passes_of_the_oracle(name):
    """orc_denoise_pass: the five passes one by one give orc_denoise's words; and the temporal pass ALONE, on FilteredOut1 words the test
    wrote (the model's), gives the model's temporal result to the recorded floor -- the stage isolated the other way round."""
    case = DC.by_name(name)
    b, whole = run_oracle(case, "exact")
    _, m = model_chain(case)
    o = O.Oracle(case.W, case.H, threads=4)
    try:
        _load_oracle(o, b)
        o.flip_parity()
        for which in ("h_refl", "v_refl", "h_diff", "v_diff", "temporal"):
            o.denoise_pass(which)
        o.tone_map()
        for key, bid in (("flt_rfl", O.BUF_FLT_RFL), ("flt_dff", O.BUF_FLT_DFF), ("tss", O.BUF_TSS0 + o.parity()), ("bb", O.BUF_BACKBUFFER)):
            np.testing.assert_array_equal(o.buffer(bid), whole[key], err_msg="%s: %s, pass by pass" % (name, key))
        assert o.L.orc_denoise_pass(o.h, 5) == -1 and o.L.orc_denoise_pass(o.h, -1) == -1, "the tone map and anything else is no pass of it"
    finally:
        o.close()
    o = O.Oracle(case.W, case.H, threads=4)
    try:
        _load_oracle(o, b)
        o.flip_parity()
        o.buffer(O.BUF_FLT_DFF, copy=False)[...] = m["flt_dff_words"]
        o.denoise_pass("temporal")
        t = m["temporal"]
        e = compare_f16(name + " temporal pass alone on the model's FilteredOut1", o.buffer(O.BUF_TSS0 + o.parity()), t["value"], where=~t["ill"], pixel_scale=True)
        check_interval(name + " temporal pass alone", o.buffer(O.BUF_TSS0 + o.parity()), t)
        recorded = json.load(open(FLOOR_PATH))["bounds"]["TemporalSSOut"]
        q = R.quantiles(e)
        print(name, q)
        assert q["max"] <= 2.0 * recorded["max"] and q["q99"] <= 1.5 * max(recorded["q99"], 0.5), q
    finally:
        o.close()


_MODEL_CACHE = {}


def model_chain(case):
    if case.name not in _MODEL_CACHE:
        b = DC.check(case)
        _MODEL_CACHE[case.name] = (b, R.chain(b))
    return _MODEL_CACHE[case.name]


def measure(case, variant):
    """Everything the module docstring lists for one case and variant; returns the entry of the floor table."""
    b, m = model_chain(case)
    _, o = run_oracle(case, variant)
    label = "%s / %s" % (case.name, variant)
    entry = {}
    # chain
    entry["FilteredOut"] = R.quantiles(compare_f16(label + " FilteredOut", o["flt_rfl"], m["flt_rfl"]))
    entry["FilteredOut1"] = R.quantiles(compare_f16(label + " FilteredOut1", o["flt_dff"], m["flt_dff"]))
    t = m["temporal"]
    entry["TemporalSSOut_chain"] = R.quantiles(compare_f16(label + " TemporalSSOut (chain)", o["tss"], t["value"], where=~t["ill"], pixel_scale=True))
    # stage isolated: the oracle's own words in
    ti = R.temporal_pass(o["flt_dff"], b["velocity"], b["history"])
    entry["TemporalSSOut"] = R.quantiles(compare_f16(label + " TemporalSSOut (fed the oracle's FilteredOut1)", o["tss"], ti["value"], where=~ti["ill"], pixel_scale=True))
    # ... and the same distance in ulps of each channel's OWN value, as FilteredOut is measured: reported beside it (denoise_ref.ulp_error says
    # why the temporal result is bounded in ulps of the pixel's largest channel)
    entry["TemporalSSOut_own_channel"] = R.quantiles(np.where(ti["ill"], -1.0, R.ulp_error(o["tss"], ti["value"])))
    check_interval(label + " TemporalSSOut", o["tss"], ti)
    entry["ill"] = int(ti["ill"].sum()); entry["long"] = int(ti["long"].sum())
    if not case.flat:
        assert entry["ill"] <= ILL_SHARE_CAP * max(entry["long"], 1), "%s: %d of %d long-path pixels ill-conditioned" % (label, entry["ill"], entry["long"])
    x, _, near = R.tone_map(o["tss"])
    differ, ties = compare_backbuffer(label + " back buffer (fed the oracle's TemporalSSOut)", o["bb"], x, near)
    entry["backbuffer"] = {"differ": differ, "near_ties": ties}
    # the chained back buffer (the model's whole chain against the oracle's): reported, not asserted -- a TemporalSSOut texel that rounds the
    # other way upstream legitimately moves a code
    d = np.abs(O.unpack_rgba8(o["bb"]).astype(np.int64) - O.unpack_rgba8(m["bb_words"]).astype(np.int64))
    entry["backbuffer_chain"] = {"differ": int((d != 0).sum()), "max_codes": int(d.max(initial=0))}
    return entry


def measure_all():
    table = {}
    for case in DC.all_cases():
        table[case.name] = {v: measure(case, v) for v in VARIANTS}
        table[case.name]["facts"] = checked_facts(case)
    return table


def checked_facts(case):
    """The case's facts from the model alone (no oracle takes part), after asserting what the case was built for."""
    facts = case_facts(case, model_chain(case)[1])
    check_expectations(case, facts)
    return facts


def floor_bounds(table):
    """Per buffer and quantile, the larger of the two variants, over all cases: what the GPU test multiplies by its margin."""
    out = {}
    for buf in ("FilteredOut", "FilteredOut1", "TemporalSSOut"):
        out[buf] = {q: max(table[c][v][buf][q] for c in table for v in VARIANTS) for q in ("max", "q999", "q99", "median")}
    return out


def write_floor():
    table = measure_all()
    doc = {"about": "binary16 ulps of the float64 model's value by which the CPU oracle's result differs from it, per case, buffer and variant of the "
                    "oracle's normal weight; written by tests/test_denoise_ref_host.py write_floor(), re-measured by every run of that module",
           "cond_max": R.COND_MAX, "k_roundings": R.K_ROUNDINGS, "cases": table, "bounds": floor_bounds(table)}
    if os.path.exists(FLOOR_PATH):
        old = json.load(open(FLOOR_PATH))
        if "gpu_measured" in old:
            doc["gpu_measured"] = old["gpu_measured"]
    with open(FLOOR_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc


def test_case_list_covers_the_sizes_and_has_one_flat_case():
    sizes = {(c.W, c.H) for c in DC.all_cases()}
    assert set(DC.SIZES) <= sizes
    assert sum(c.flat for c in DC.all_cases()) == 1, "one flat case, the only one exempt from the ill-conditioned cap"


@pytest.mark.parametrize("name", DC.NAMES)
def test_model_against_oracle_and_recorded_floor(name):
    case = DC.by_name(name)
    recorded = json.load(open(FLOOR_PATH))
    assert recorded["cond_max"] == R.COND_MAX and recorded["k_roundings"] == R.K_ROUNDINGS
    # integer facts of the case (the model's alone): exactly
    assert checked_facts(case) == recorded["cases"][name]["facts"], "%s: the case's facts moved" % name
    for variant in VARIANTS:
        got, want = measure(case, variant), recorded["cases"][name][variant]
        print("%s / %s: %s" % (name, variant, json.dumps(got)))
        assert (got["ill"], got["long"]) == (want["ill"], want["long"]), "%s / %s: excluded share moved" % (name, variant)
        for buf in ("FilteredOut", "FilteredOut1", "TemporalSSOut", "TemporalSSOut_chain", "TemporalSSOut_own_channel"):
            assert got[buf]["n"] == want[buf]["n"], "%s / %s %s: number of compared pixels" % (name, variant, buf)
            for q in ("max", "q999", "q99", "median"):
                if variant == "exact":
                    assert got[buf][q] == pytest.approx(want[buf][q], rel=1e-9, abs=1e-12), "%s / exact %s %s: the floor moved" % (name, buf, q)
                else:   # libm: the host's C library takes part
                    assert abs(got[buf][q] - want[buf][q]) <= LIBM_DRIFT_ULPS, "%s / libm %s %s: %.3f recorded %.3f" % (name, buf, q, got[buf][q], want[buf][q])
        if variant == "exact":
            assert got["backbuffer"] == want["backbuffer"]


def test_recorded_bounds_follow_from_the_recorded_cases():
    recorded = json.load(open(FLOOR_PATH))
    assert recorded["bounds"] == floor_bounds(recorded["cases"])
    assert sorted(recorded["cases"]) == sorted(DC.NAMES)
