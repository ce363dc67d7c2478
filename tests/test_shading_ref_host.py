"""The float64 model of the shading path (tests/shading_ref.py) on the CPU, no GPU:

  a  known answers no implementation is witness of: both half-vector maps have the densities they are said to have (finite-difference
     Jacobians); weight x pdf = BRDF x NoL; a constant cube's answers; the eye-ray barycentrics at projected vertices and centroid;
  b  the model against the CPU oracle, per pixel, on every case of tests/shading_cases.py: the restatement that returns the two traced
     images and the primary surface in fp32, in front of their packs.  On unflagged pixels the pattern of "no ray traced" and the
     non-finite pattern coincide, the fp32 values are measured against the model's interval in fp32 ulps -- THE FLOOR, recorded in
     tests/golden/shading_synthetic_floor.json and re-measured by every run -- and every stored word obeys
  c  the code rule: a stored code differs from the code of the model's value by at most one, and only where that value lies within delta
     of a rounding boundary; delta = the family's recorded maximum floor x MARGIN, in the format's units.
  The share of flagged pixels is at most FLAG_CAP of the covered ones, in every frame of every case.

tests/test_gpu_shading_synthetic.py runs the same cases on the device and takes check_words and the recorded floor from here.
Regenerate the floor by hand after a deliberate change of the model, the oracle or the cases (the `gpu_measured` entry is kept):

    python -c "import sys; sys.path[:0] = ['tests', '.']; import test_shading_ref_host as t; t.write_floor()"

  d  the sun's and the local lights' passes (families sun and lights), stage by stage: their restatements (tests/lights_ref.py, which
     carries both settings) expose no fp32 value in front of the pack, so the model's pass is given the oracle's words as they stand in
     front of the pass, adds its term to the unpacked word and the code rule is asked of the word behind the pass (check_direct_stage);
     delta from the floor the same scenes' ray-traced path records.  Words the pass must not touch stay bit for bit."""
import json
import os

import numpy as np
import pytest

import lights_ref as LR
import restatement as RS
import sun_ref as SR
import shading_cases as SC
import shading_ref as R
from oracle import oracle as O

FLOOR_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_synthetic_floor.json")
FLAG_CAP = 0.02
MARGIN = 2.0                      # on a recorded maximum; the project caps it at 4
UNIT = 2.0 ** -23                 # the G-buffer's values are measured in fp32 ulps of 1: normals, velocities and roughness live in [-1, 1]
QUANTS = ("max", "q99", "median")
# The floor's maximum is set by the smallest roughness codes (the samplers' cancelling roots, shading_ref.CANCEL_SLACK), so it is recorded twice:
# over all pixels, and over those whose primary surface has a roughness of at least ROUGH_CLASS ("max_rough") -- and a pixel's delta comes from
# its own class.  Nothing drawn counts as rough: the sky has no sampler.
ROUGH_CLASS = 0.05
FLOOR_DRIFT = 1.25                # a re-measured figure may exceed the recorded one by this factor (another libm, numpy or compiler moves last bits)
GRAZING_NOL_ERROR = 1e-5         # absolute error of NoL in fp32: the screen-space barycentrics' few 1e-6, doubled by the reflection, with room
RELAXED_VELOCITY_CAP = 0.25       # of a frame's velocity values may lie below 2^10 delta, where binary16 is finer than delta (check_words)


# ---- running a case ----------------------------------------------------------------------------------------------------------------
def load_oracle(o, case):
    for slot, (v, i) in enumerate(case.meshes):
        o.set_mesh(slot, v, i)
    o.set_env_rgba16f(case.cube.size, case.cube.mips, case.cube.mip_major())
    o.set_sampler(case.vndf)


def oracle_words(o):
    return {"vis": o.buffer(O.BUF_VISIBILITY), "normal": o.buffer(O.BUF_NORMAL), "rm": o.buffer(O.BUF_ROUGH_METAL), "velocity": o.buffer(O.BUF_VELOCITY),
            "refl": o.buffer(O.BUF_RT_REFL), "diff": o.buffer(O.BUF_RT_DIFF)}


def run_oracle(case, lib=None):
    """Every frame of a case on the oracle -> per frame the words, and (own library only) rays and the fp32 values in front of the packs."""
    o = RS.Oracle(case.W, case.H, threads=4, depth=1, samples=1, entry="spp") if lib is None else O.Oracle(case.W, case.H, threads=4, lib=lib)
    try:
        load_oracle(o, case)
        o.build_as(); o.transform_sh()
        out = []
        for k in range(len(SC.FRAMES)):
            o.set_frame_constants(case.constants(k)); o.update_as(); o.render_visibility()
            if lib is None:
                rays, refl, diff, primary = o.ray_trace_primary_f32()
                f = dict(oracle_words(o), rays=rays, refl_f32=refl, diff_f32=diff, primary_f32=primary)
            else:
                f = dict(oracle_words(o), rays=o.ray_trace())
                f.update(oracle_words(o))
            out.append(f)
        return out
    finally:
        o.close()


_MODEL = {}


def model_frames(case, vis_per_frame):
    """The model's frames of a case, computed once per process; the visibility words are its input and must be the ones it was computed for."""
    if case.name not in _MODEL:
        scene, prev, frames = R.Scene(case.meshes, case.cube), None, []
        for k, vis in enumerate(vis_per_frame):
            prev = R.frame(scene, case.constants(k), vis, case.W, case.H, case.vndf, prev)
            prev["vis"] = np.array(vis)
            frames.append(prev)
        _MODEL[case.name] = frames
    for m, vis in zip(_MODEL[case.name], vis_per_frame):
        np.testing.assert_array_equal(m["vis"], vis, err_msg="%s: the visibility words differ from those the model was run on" % case.name)
    return _MODEL[case.name]


# ---- c: the code rule on a frame's words (the GPU test's assertion too) ---------------------------------------------------------------
def check_words(label, w, m, prev_w, bounds):
    """Asserts the code rule for the five words of one frame against the model m on unflagged pixels, and the carry-over bit for bit.
    bounds: the family's recorded floor.  -> {word: (values that used the one-code allowance, values compared)}."""
    ok = m["flags"] == 0
    used = {}

    def rule(name, code_of, stored, lo, hi, delta, where, one_code=True):
        bad, allowance = R.code_rule(code_of, stored, lo, hi, delta, one_code)
        where = np.broadcast_to(where.reshape(where.shape + (1,) * (bad.ndim - where.ndim)), bad.shape)
        at = np.argwhere(bad & where)
        assert at.size == 0, "%s: %s breaks the code rule at %d values, first (y, x, channel) %s: stored code %s, the model's value in [%s, %s]" % (
            label, name, len(at), at[0].tolist(), np.asarray(stored)[tuple(at[0])], np.asarray(lo)[tuple(at[0])], np.asarray(hi)[tuple(at[0])])
        used[name] = (int((allowance & where).sum()), int(where.sum()))

    dg, dv = bounds["gbuffer"]["max"] * MARGIN * UNIT, bounds["velocity"]["max"] * MARGIN * UNIT
    rough_class = (m["rm_value"][..., 0] >= ROUGH_CLASS) | ~m["covered"]
    nw = np.asarray(w["normal"]).astype(np.int64)
    rule("normal", lambda x: R.unorm_code(x, 1023), np.stack([nw & 1023, (nw >> 10) & 1023, (nw >> 20) & 1023], axis=-1), m["normal_value"], m["normal_value"], dg, ok)
    np.testing.assert_array_equal(nw >> 30, np.where(m["covered"], 3, 0), err_msg="%s: the normal word's hit bits" % label)
    rw = np.asarray(w["rm"]).astype(np.int64)
    known = ok & (m["covered"] if prev_w is None else np.ones_like(ok))      # (nothing drawn yet: the word is whatever the buffer held)
    rule("rough_metal", lambda x: R.unorm_code(x, 255), np.stack([rw & 255, rw >> 8], axis=-1), m["rm_value"], m["rm_value"], dg, known & m["covered"])
    vw = np.asarray(w["velocity"]).astype(np.int64)
    rule("velocity", R.f16_ordered, np.stack([R.f16_words_ordered(vw & 0xFFFF), R.f16_words_ordered(vw >> 16)], axis=-1), m["velocity_value"], m["velocity_value"], dv, ok,
         one_code=R.f16_spacing(m["velocity_value"]) >= dv)      # (a velocity below 2^10 delta: binary16 is finer there than fp32's error of the difference it is)
    relaxed = float((R.f16_spacing(m["velocity_value"]) < dv)[m["covered"]].mean()) if m["covered"].any() else 0.0
    used["velocity_relaxed"] = (int((R.f16_spacing(m["velocity_value"]) < dv)[m["covered"]].sum()), 2 * int(m["covered"].sum()))
    assert relaxed <= RELAXED_VELOCITY_CAP, "%s: %.1f %% of the velocity values lie where binary16 is finer than delta: move the case's camera, not the cap" % (label, 100 * relaxed)
    for name, key, where in (("RayTracingOut0", "refl", ok), ("RayTracingOut1", "diff", ok & m["diff_written"])):
        lo, hi = np.where(where[..., None], m[key + "_lo"], 0.0), np.where(where[..., None], m[key + "_hi"], 0.0)
        delta = np.where(rough_class, bounds[key]["max_rough"], bounds[key]["max"])[..., None] * MARGIN * R.ulp32(np.maximum(np.abs(lo), np.abs(hi)).max(axis=-1))[..., None]
        stored = R.r11g11b10_split(w[key])
        for ch, mb in enumerate((6, 6, 5)):
            rule("%s channel %d" % (name, ch), lambda x, mb=mb: R.ufloat_code(x, mb), stored[..., ch], lo[..., ch], hi[..., ch], delta[..., 0], where)
    if prev_w is not None:      # what a frame does not write stays, bit for bit
        np.testing.assert_array_equal(w["diff"][~m["diff_written"]], prev_w["diff"][~m["diff_written"]], err_msg="%s: RayTracingOut1 carried over" % label)
        np.testing.assert_array_equal(w["rm"][~m["covered"]], prev_w["rm"][~m["covered"]], err_msg="%s: the rough-metal word carried over" % label)
    return used


def light_dicts(lights):
    """The lights as the host hands them on (fp32, the axis normalised): what both the device's pass and the model see."""
    return [dict(position=f[0:3], range=f[3], intensity=f[4:7], radius=float(f[7]), axis=f[8:11], cos_outer=f[11], cos_inner=f[12]) for f in LR.records(lights)]


def direct_passes(case, k, scene, m):
    """The model's passes of frame position k in the order the frame runs them: [(name, pass result)]."""
    out = []
    if case.sun is not None:
        d, e = case.sun(k)
        out.append(("sun", R.sun_pass(scene, case.constants(k), m, SR.normalise(d), e)))
    if case.lights is not None:
        out.append(("lights", R.lights_pass(scene, case.constants(k), m, light_dicts(case.lights(k)))))
    return out


def check_direct_stage(label, before, after, p, bounds):
    """One pass against the model: the words `after` it from the words `before` it.  -> {image: (allowance used, values compared)}."""
    ok = p["flags"] == 0
    used = {}
    for name, key, lo_t, hi_t, where in (("RayTracingOut0", "refl", p["spec_lo"], p["spec_hi"], p["term"]),
                                         ("RayTracingOut1", "diff", p.get("diff_lo", p["diff"]), p.get("diff_hi", p["diff"]), p["diffuse"])):
        base = R.unpack_r11g11b10(before[key])
        lo, hi = base + lo_t, base + hi_t
        delta = bounds[key]["max"] * MARGIN * R.ulp32(np.maximum(np.abs(lo), np.abs(hi)).max(axis=-1))
        stored = R.r11g11b10_split(after[key])
        a_sum = 0
        for ch, mb in enumerate((6, 6, 5)):
            bad, allowance = R.code_rule(lambda x, mb=mb: R.ufloat_code(x, mb), stored[..., ch], lo[..., ch], hi[..., ch], delta)
            at = np.argwhere(bad & ok & where)
            assert at.size == 0, "%s: %s channel %d breaks the code rule at %d values, first (y, x) %s: stored code %s, the model's value in [%s, %s]" % (
                label, name, ch, len(at), at[0].tolist(), stored[..., ch][tuple(at[0])], lo[..., ch][tuple(at[0])], hi[..., ch][tuple(at[0])])
            a_sum += int((allowance & ok & where).sum())
        used[name] = (a_sum, 3 * int((ok & where).sum()))
        still = ok & ~where
        np.testing.assert_array_equal(after[key][still], before[key][still], err_msg="%s: %s changed where the pass adds nothing" % (label, name))
    return used


def run_direct_oracle(case):
    """Every frame of a sun / lights case on the restatement that carries both settings, pass by pass: per frame [(name, words, rays)], the
    first entry the frame in front of the passes."""
    o = LR.Oracle(case.W, case.H, threads=4)
    try:
        load_oracle(o, case)
        o.build_as(); o.transform_sh()
        out = []
        for k in range(len(SC.FRAMES)):
            o.set_frame_constants(case.constants(k)); o.update_as(); o.render_visibility()
            o.set_sun(None, None); o.set_lights([])
            rays = o.ray_trace()
            stages = [("base", oracle_words(o), rays)]
            if case.sun is not None:
                o.set_sun(*case.sun(k))
                rays = o.sun_apply()
                stages.append(("sun", oracle_words(o), rays))
            if case.lights is not None:
                o.set_lights(case.lights(k))
                rays = o.lights_apply()
                stages.append(("lights", oracle_words(o), rays))
            out.append(stages)
        return out
    finally:
        o.close()


def check_direct(case, frames_of_stages):
    """Assertions d on the stages of every frame (the oracle's, or the device's).  -> allowance counts, and what the passes did."""
    scene = R.Scene(case.meshes, case.cube)
    models = model_frames(case, [st[0][1]["vis"] for st in frames_of_stages])
    bounds = recorded()["bounds"][case.family]
    used, facts = {}, {"terms": 0, "rays": 0, "flags": 0, "flagged": 0}
    for k, (stages, m) in enumerate(zip(frames_of_stages, models)):
        for (name, p), before, after in zip(direct_passes(case, k, scene, m), stages[:-1], stages[1:]):
            assert after[0] == name
            label = "%s frame %d, the %s pass" % (case.name, SC.FRAMES[k], name)
            share = float(((p["flags"] != 0) & m["covered"]).sum()) / max(int(m["covered"].sum()), 1)
            assert share <= FLAG_CAP, "%s: %.2f %% of the covered pixels flagged" % (label, 100 * share)
            n_flagged = int((p["flags"] != 0).sum())
            assert after[2] is None or abs(after[2] - p["rays"]) <= len(case.lights(k) if name == "lights" else [0]) * n_flagged, "%s: %s shadow rays, the model %d" % (label, after[2], p["rays"])
            for img, (a, b) in check_direct_stage(label, before[1], after[1], p, bounds).items():
                t = used.setdefault(name + " " + img, [0, 0]); t[0] += a; t[1] += b
            facts["terms"] += int(p["term"].sum()); facts["rays"] += p["rays"]; facts["flags"] |= int(np.bitwise_or.reduce(p["flags"].reshape(-1)))
    return used, facts


def flagged_share(m):
    return float(((m["flags"] != 0) & m["covered"]).sum()) / max(int(m["covered"].sum()), 1)


# ---- b: the model against the oracle's fp32 values -----------------------------------------------------------------------------------
def measure(case):
    """Asserts b on every frame; returns the case's entry of the floor table."""
    frames = run_oracle(case)
    models = model_frames(case, [f["vis"] for f in frames])
    e = {"refl": [], "diff": [], "gbuffer": [], "velocity": []}
    rough_e = {"refl": [], "diff": []}
    flags_seen, share, carried, grazing = 0, 0.0, 0, 0
    for k, (f, m) in enumerate(zip(frames, models)):
        label = "%s frame %d" % (case.name, SC.FRAMES[k])
        ok, cov = m["flags"] == 0, m["covered"]
        assert cov.mean() >= 0.05, "%s: next to nothing is drawn" % label
        share = max(share, flagged_share(m))
        assert flagged_share(m) <= FLAG_CAP, "%s: %.2f %% of the covered pixels are flagged (%s): change the case, not the cap" % (
            label, 100 * flagged_share(m), {n: int(((m["flags"] & b) != 0).sum()) for b, n in R.FLAG_NAMES.items()})
        flags_seen |= int(np.bitwise_or.reduce(m["flags"].reshape(-1)))
        n_flagged = int((~ok).sum())
        assert abs(f["rays"] - m["rays"]) <= 2 * n_flagged, "%s: %d rays, the model traces %d (%d pixels flagged)" % (label, f["rays"], m["rays"], n_flagged)
        untraced = ok & cov & ~m["refl_traced"]
        assert (f["refl_f32"][untraced] == 0.0).all(), "%s: a value where the model traces no reflection ray" % label
        traced_somewhere = ok & cov & m["refl_traced"] & (np.abs(m["refl_lo"]).max(axis=-1) > 1e-6)
        assert (np.abs(f["refl_f32"][traced_somewhere]).max(axis=-1) > 0.0).all(), "%s: zero where the model traces a reflection ray" % label
        assert np.isnan(f["diff_f32"][cov & ~m["diff_traced"]]).all() and not np.isnan(f["diff_f32"][ok & m["diff_written"]]).any(), "%s: the diffuse rays' pattern" % label
        for key, where in (("refl", ok), ("diff", ok & m["diff_written"])):
            assert np.isfinite(f[key + "_f32"][where]).all() and np.isfinite(m[key + "_lo"][where]).all() and np.isfinite(m[key + "_hi"][where]).all(), "%s: non-finite %s" % (label, key)
            e[key].append(R.ulp_distance(f[key + "_f32"][where], m[key + "_lo"][where], m[key + "_hi"][where]))
            rough_e[key].append(e[key][-1][((m["rm_value"][..., 0] >= ROUGH_CLASS) | ~cov)[where]])
        # pixels flagged for a grazing reflection and nothing else leave the ulp comparison, not the test: their value is C NoL, so the oracle
        # may differ from the model's hull by C x GRAZING_NOL_ERROR = value x GRAZING_NOL_ERROR / NoL (and the well-conditioned pixels' recorded floor)
        gz = (m["flags"] == R.FLAG_GRAZING) & cov
        if gz.any():
            hi_abs = np.maximum(np.abs(m["refl_lo"][gz]), np.abs(m["refl_hi"][gz])).max(axis=-1)
            dist = np.maximum(np.maximum(m["refl_lo"][gz] - f["refl_f32"][gz], f["refl_f32"][gz] - m["refl_hi"][gz]), 0.0).max(axis=-1)
            allowed = hi_abs * GRAZING_NOL_ERROR / m["refl_nol"][gz] + MARGIN * recorded()["bounds"][case.family]["refl"]["max"] * R.ulp32(hi_abs)
            assert (dist <= allowed).all(), "%s: a grazing reflection is off by %.3g, allowed %.3g" % (label, dist[np.argmax(dist - allowed)], allowed[np.argmax(dist - allowed)])
            grazing += int(gz.sum())
        g = np.concatenate([m["normal_value"], m["velocity_value"], m["rm_value"][..., :1]], axis=-1)
        e["gbuffer"].append((np.abs(f["primary_f32"].astype(np.float64) - g)[ok & cov].max(axis=-1, initial=0.0) if (ok & cov).any() else np.zeros(0)) / UNIT)
        e["gbuffer"].append(np.abs(f["primary_f32"].astype(np.float64)[..., :5] - g[..., :5])[ok & ~cov].max(axis=-1) / UNIT)
        e["velocity"].append(np.abs(f["primary_f32"].astype(np.float64)[..., 3:5] - m["velocity_value"])[ok].max(axis=-1) / UNIT)
        carried += int((cov & ~m["diff_written"]).sum()) + int((~cov).sum()) if k else 0
    entry = {key: R.quantiles(np.concatenate(v)) for key, v in e.items()}
    for key, v in rough_e.items():
        entry[key]["max_rough"] = float(np.concatenate(v).max(initial=0.0))
    entry.update(family=case.family, flagged_share_max=share, flags_seen=sorted(n for b, n in R.FLAG_NAMES.items() if flags_seen & b), carried_over=carried)
    return entry, frames, models


def floor_bounds(cases):
    out = {}
    for fam in SC.FAMILIES:
        mine = [c for c in cases.values() if c["family"] == fam]
        out[fam] = {key: {q: max(c[key][q] for c in mine) for q in QUANTS + (("max_rough",) if key in ("refl", "diff") else ())} for key in ("refl", "diff", "gbuffer", "velocity")}
    return out


# What dominates each family's floor (read from the worst pixels when the floor was first measured).
DOMINATES = {
    "transforms": "reflection: the NDF map's root of 1 - cos^2 theta at roughness 0.16 and 0.5 x 0.25 (inside the model's hull, the rest of it outside); both images: "
                  "the primary surface's barycentrics from screen-space gradients, carried into P, V and the directions, times the cube's slope",
    "normals": "reflection: NoL of a few 1e-3 on normals turned away from the eye (relative error = absolute error of NoL over NoL, just above the grazing flag's 2^-8)",
    "materials": "reflection: roughness codes 1/255 to 0.05 (alpha^2 down to 2e-10: the half vector's tilt is rounding noise of 1 - cos^2 theta) seen through the "
                 "checkerboard and the room's corners; diffuse: the SH sum's cancellation under the signed cube",
    "hits": "reflection: as transforms; the apex pixel and the coincident sheets add nothing",
    "sun": "reflection: as transforms on the slab's checkerboard (roughness 0.025); the sun's own pass is held through the words, its GGX denominator as an interval",
    "lights": "reflection: as transforms; the lights' pass is held through the words",
    "vndf": "reflection: the root of 1 - t1^2 - t2^2 near the disk's rim, otherwise as materials and normals",
}


def write_floor():
    cases = {c.name: measure(c)[0] for c in SC.all_cases()}
    doc = {"about": "fp32 ulps (of the pixel's largest channel; the G-buffer's values: of 1) by which the CPU oracle's values in front of their packs differ from the "
                    "float64 model's interval, unflagged pixels, all frames of a case; written by tests/test_shading_ref_host.py write_floor(), re-measured by every "
                    "run of that module", "margin": MARGIN, "flag_cap": FLAG_CAP, "cancel_slack": R.CANCEL_SLACK, "grazing_nol": R.GRAZING_NOL,
           "cases": cases, "bounds": floor_bounds(cases), "dominates": DOMINATES}
    if os.path.exists(FLOOR_PATH):
        old = json.load(open(FLOOR_PATH))
        if "gpu_measured" in old:
            doc["gpu_measured"] = old["gpu_measured"]
    with open(FLOOR_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc


def recorded():
    return json.load(open(FLOOR_PATH))


@pytest.mark.parametrize("name", SC.NAMES)
def test_model_against_oracle_and_recorded_floor(name):
    case = SC.by_name(name)
    rec = recorded()
    assert (rec["cancel_slack"], rec["grazing_nol"], rec["margin"], rec["flag_cap"]) == (R.CANCEL_SLACK, R.GRAZING_NOL, MARGIN, FLAG_CAP)
    got, frames, models = measure(case)
    print("%s: %s" % (name, json.dumps(got)))
    want = rec["cases"][name]
    assert (got["family"], got["flags_seen"], got["carried_over"]) == (want["family"], want["flags_seen"], want["carried_over"])
    assert got["flagged_share_max"] <= FLAG_CAP
    for key in ("refl", "diff", "gbuffer", "velocity"):
        assert got[key]["n"] == want[key]["n"], "%s %s: number of compared pixels" % (name, key)
        for q in want[key]:
            if q != "n":      # a measurement: last bits of libm and numpy move it; what is asked is that it has not grown
                assert got[key][q] <= FLOOR_DRIFT * want[key][q] + 0.5, "%s %s %s: the floor grew: %.3f, recorded %.3f" % (name, key, q, got[key][q], want[key][q])
    prev = None
    for k, (f, m) in enumerate(zip(frames, models)):
        check_words("%s frame %d" % (name, SC.FRAMES[k]), f, m, prev, rec["bounds"][case.family])
        prev = f


def test_recorded_bounds_follow_from_the_recorded_cases_and_the_cases_reach_their_branches():
    rec = recorded()
    assert sorted(rec["cases"]) == sorted(SC.NAMES) and rec["bounds"] == floor_bounds(rec["cases"])
    assert sorted(rec["dominates"]) == sorted(SC.FAMILIES)
    seen = set().union(*(c["flags_seen"] for c in rec["cases"].values()))
    assert {"up", "checker", "grazing"} <= seen, "no case comes near the up-vector switch, a checkerboard step or a grazing reflection: %s" % sorted(seen)
    assert sum(c["carried_over"] > 0 for c in rec["cases"].values()) >= 2, "the carry-over of RayTracingOut1 and of the rough-metal word is seen nowhere"
    sizes = {(c.W, c.H) for c in SC.all_cases()}
    assert (75, 53) in sizes and max(w for w, _ in sizes) <= 96 and max(h for _, h in sizes) <= 64


def test_cases_visit_what_they_were_built_for():
    """Facts of the cases from their constants alone (no oracle, no model frame)."""
    c = SC.by_name("skew_75x53")
    fc = R.read_constants(c.constants(1))
    for w in fc["world"]:
        it = R.inverse_transpose(w)
        n = np.array([0.3, 0.8, 0.5])
        a, b = n @ it, n @ w[:3, :3]
        assert np.abs(np.cross(a / np.linalg.norm(a), b / np.linalg.norm(b))).max() > 0.05, "World and its inverse transpose turn a normal the same way"
    assert np.linalg.det(R.read_constants(SC.by_name("mirrored_bias_75x53").constants(0))["world"][1][:3, :3]) < 0
    assert np.abs(R.read_constants(SC.by_name("mirrored_bias_75x53").constants(0))["proj_bias"]).min() > 0
    # a previous position off screen: the velocity word's definition turned round, on the model's frame
    m = model_frames(c, [f["vis"] for f in run_oracle(c)])[1]
    py, px = np.divmod(np.arange(c.W * c.H), c.W)
    ndc = np.stack([(px + 0.5) / c.W * 2 - 1, -((py + 0.5) / c.H * 2 - 1)], axis=1).reshape(c.H, c.W, 2)
    before = ndc - m["velocity_value"] * [2.0, -2.0]
    assert (np.abs(before).max(axis=-1)[m["covered"]] > 1.0).any(), "no covered pixel's previous position is off screen"
    rough = sorted({float(np.float32(SC.by_name("materials_%d_64x48" % i).materials(k)[1][1])) for i in range(4) for k in range(3)})
    assert len(rough) == 12 and rough[0] == float(np.float32(1 / 255)) and rough[-1] == 1.0
    assert any(SC.by_name("materials_%d_64x48" % i).materials(k)[0][1] == 0.0 for i in range(4) for k in range(3))
    metals = {(SC.by_name("materials_%d_64x48" % i).materials(0)[0][2] > 0.5, SC.by_name("materials_%d_64x48" % i).materials(0)[1][2] > 0.5) for i in range(4)}
    assert len(metals) == 4
    assert {len(SC.by_name("materials_%d_64x48" % i).cube.levels) for i in range(4)} == {1, 3, 5}
    n = SC.by_name("normals_75x53").meshes[1][0][:, 4]
    assert (n == 1.0).any() and (n == -1.0).any() and ((np.abs(n) < 0.999) & (np.abs(n) > 0.998)).any() and ((np.abs(n) >= 0.999) & (np.abs(n) < 1.0)).any()


@pytest.mark.parametrize("name", [c.name for c in SC.all_cases() if c.sun is not None or c.lights is not None])
def test_sun_and_lights_passes_against_the_model(name):
    case = SC.by_name(name)
    used, facts = check_direct(case, run_direct_oracle(case))
    print("%s: %s %s" % (name, json.dumps(used), facts))
    assert facts["terms"] > 1000 and facts["rays"] > facts["terms"] + 100, "%s: too few terms, or nothing occluded: %s" % (name, facts)
    assert all(b > 0 for _, b in used.values())


def test_sun_and_light_terms_by_hand():
    c, E = np.array([0.8, 0.4, 0.2]), np.array([3.0, 2.0, 1.0])
    s = {"N": np.array([[0.0, 1.0, 0.0]]), "V": R._unit(np.array([[0.3, 0.9, 0.1]])), "rough": np.array([0.5]), "metal": np.array([0.0]), "colour": c[None]}
    L = np.array([[np.sqrt(0.75), 0.5, 0.0]])
    _, _, diff = R._direct_term(s, np.array([0]), L, np.array([0.5]))
    np.testing.assert_allclose(diff[0] * E, c * 0.96 * 0.5 / np.pi * E, rtol=1e-14)      # a slab facing a sun of irradiance E at NoL = 0.5
    s["metal"] = np.array([1.0])
    assert (R._direct_term(s, np.array([0]), L, np.array([0.5]))[2] == 0).all()
    # roughness below 1 / 32 is lifted to it
    lo_a, hi_a, _ = R._direct_term(dict(s, rough=np.array([0.001])), np.array([0]), L, np.array([0.5]))
    lo_b, hi_b, _ = R._direct_term(dict(s, rough=np.array([1.0 / 32.0])), np.array([0]), L, np.array([0.5]))
    np.testing.assert_array_equal(lo_a, lo_b); np.testing.assert_array_equal(hi_a, hi_b)
    # the window: 0 at d = R, within 3 % of 1 at d = R / 3; att d^2 -> 1 as d / R -> 0; the spot factor a quarter halfway between the cones
    Rr = 7.0
    assert R.light_window(Rr * Rr, Rr) == 0.0 and abs(R.light_window((Rr / 3) ** 2, Rr) - 1.0) < 0.03
    ratio = [float(R.light_attenuation(np.array([(Rr * x) ** 2]), Rr)[0] * (Rr * x) ** 2) for x in (0.3, 0.1, 0.03, 0.01)]
    assert all(a < b for a, b in zip(ratio, ratio[1:])) and abs(ratio[-1] - 1.0) < 1e-7
    assert R.light_spot(0.5 * (0.9 + 0.6), 0.6, 0.9) == pytest.approx(0.25, abs=1e-15)
    assert float(R.light_attenuation(np.array([1e-6]), 1.0)[0]) == pytest.approx(1e4, rel=1e-9)      # the floor m2 = 1e-4 below d = 0.01


# ---- a: known answers ----------------------------------------------------------------------------------------------------------------
def _density_by_jacobian(h_of, u, v, step):
    """1 / |dh/du x dh/dv| by central differences: the density on the sphere of the image of the uniform density on the unit square."""
    du = (h_of(u + step, v) - h_of(u - step, v)) / (2 * step)
    dv = (h_of(u, v + step) - h_of(u, v - step)) / (2 * step)
    return 1.0 / np.linalg.norm(np.cross(du, dv), axis=1)


@pytest.mark.parametrize("alpha", [0.01, 0.25, 1.0])
@pytest.mark.parametrize("cos_view", [0.95, 0.5, 0.1])
def test_both_half_vector_maps_have_their_stated_densities(alpha, cos_view):
    g = np.linspace(0.1, 0.9, 9)
    u, v = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    N = np.tile([0.36, 0.48, 0.8], (u.size, 1))
    T, B, _ = R.tangent_frame(N)
    V = np.sqrt(1 - cos_view ** 2) * (0.6 * T + 0.8 * B) + cos_view * N
    al = np.full(u.size, alpha)
    maps = {"ndf": lambda a, b: R.ndf_half_vector(N, al, 2 * np.pi * a, b)[0], "vndf": lambda a, b: R.vndf_half_vector(N, V, al, 2 * np.pi * a, b)[0]}
    for name, h_of in maps.items():
        h = h_of(u, v)
        NoH, VoH, NoV = R._dot(N, h), R._dot(V, h), R._dot(N, V)
        want = R.ggx_d(al, NoH) * NoH if name == "ndf" else R.g1(al, NoV) * np.maximum(VoH, 0.0) * R.ggx_d(al, NoH) / NoV
        step = 1e-4
        coarse, fine = _density_by_jacobian(h_of, u, v, step), _density_by_jacobian(h_of, u, v, step / 2)
        tol = 2.0 * np.abs(coarse - fine) + 1e-7 * np.abs(fine)      # the difference's own error: a second-order scheme loses 3/4 of it by halving the step
        assert (np.abs(fine - want) <= tol).all(), "%s map, alpha %g, NoV %g: density off by up to %.3g (relative), allowed %.3g" % (
            name, alpha, cos_view, np.max(np.abs(fine - want) / want), np.max(tol / want))


def test_weight_times_pdf_is_brdf_times_nol():
    rng = np.random.default_rng(3)
    n = 500
    N = np.tile([0.0, 0.0, 1.0], (n, 1))
    V, h = R._unit(rng.normal(size=(n, 3)) + [0, 0, 1.5]), R._unit(rng.normal(size=(n, 3)) + [0, 0, 2.0])
    L = 2.0 * R._dot(V, h)[:, None] * h - V
    keep = (V[:, 2] > 0.05) & (L[:, 2] > 0.05) & (R._dot(V, h) > 0.05)
    V, h, L, N = V[keep], h[keep], L[keep], N[keep]
    al = rng.uniform(0.01, 1.0, len(V))
    f0 = R.f0_of(rng.uniform(0, 1.5, (len(V), 3)), rng.uniform(0, 1, len(V)))
    NoV, NoL, NoH, VoH = V[:, 2], L[:, 2], h[:, 2], R._dot(V, h)
    brdf_nol = R.fresnel(f0, VoH) * (R.ggx_d(al, NoH) * R.vis_smith(al, NoV, NoL) * NoL)[:, None]
    pdf_ndf = R.ggx_d(al, NoH) * NoH / (4 * VoH)
    pdf_vndf = R.g1(al, NoV) * VoH * R.ggx_d(al, NoH) / NoV / (4 * VoH)
    np.testing.assert_allclose(R.ndf_weight(f0, al, NoV, NoL, VoH, NoH) * pdf_ndf[:, None], brdf_nol, rtol=1e-12, atol=0)
    np.testing.assert_allclose(R.vndf_weight(f0, al, NoL, VoH) * pdf_vndf[:, None], brdf_nol, rtol=1e-12, atol=0)
    # F at its ends: F0 head on; sat(50 F0.g) at grazing
    np.testing.assert_allclose(R.fresnel(np.array([[0.04, 0.04, 0.04]]), np.array([1.0])), [[0.04] * 3])
    np.testing.assert_allclose(R.fresnel(np.array([[0.5, 0.01, 0.2]]), np.array([0.0])), [[0.5] * 3])


def test_a_constant_cube_gives_its_radiance_back():
    cube = SC.constant_cube()
    scene = R.Scene([SC.grid(1, 1, -1, 1, -1, 1), SC.grid(1, 1, -1, 1, -1, 1)], cube)
    Lr = 1.5
    N = R._unit(np.random.default_rng(1).normal(size=(50, 3)))
    colour = np.array([0.3, 0.0, 1.2])
    np.testing.assert_allclose(R.sh_irradiance(scene.sh, N) / np.pi * colour, np.tile(colour * Lr, (50, 1)), rtol=1e-9, atol=1e-12)      # irradiance pi L
    lo, hi = scene.environment(N, 0.7)
    np.testing.assert_allclose(lo, Lr, rtol=1e-14); np.testing.assert_allclose(hi, Lr, rtol=1e-14)
    # a metallic-1 hit: L EnvBRDFApprox, the approximation worked out by hand at roughness 0.5, NoV 1, F0 = (1, 0.5, 0.004)
    rx, ry, rz, rw = 0.5, 0.02875, 0.754, -0.029
    a004 = min(rx * rx, 2.0 ** -9.28) * rx + ry
    A, B = -1.04 * a004 + rz, 1.04 * a004 + rw
    f0 = np.array([[1.0, 0.5, 0.004]])
    want = np.array([1.0 * A + B, 0.5 * A + B, 0.004 * A + B])      # sat(50 x 0.5) = 1
    np.testing.assert_allclose(R.env_brdf_approx(f0, np.array([0.5]), np.array([1.0]))[0], want, rtol=1e-14)
    dark_green = np.array([[1.0, 0.004, 0.5]])      # sat(50 x 0.004) = 0.2 scales the bias term
    np.testing.assert_allclose(R.env_brdf_approx(dark_green, np.array([0.5]), np.array([1.0]))[0], dark_green[0] * A + 0.2 * B, rtol=1e-14)


def test_eye_ray_barycentrics_at_projected_vertices_and_centroid():
    vp = SC.look_at((0.2, 0.3, -1.0), (0.0, 0.0, 4.0)) @ SC.perspective(1.0, 1.4, 0.1, 100.0)
    tri = np.array([[-1.0, -0.5, 0.6], [1.5, 0.2, 9.0], [0.3, 1.2, 30.0]])      # steep: depths 1.6 to 31 from the eye
    pts = np.concatenate([tri, tri.mean(axis=0, keepdims=True)])
    clip = np.concatenate([pts, np.ones((4, 1))], axis=1) @ vp
    ndc = clip[:, :2] / clip[:, 3:]
    b = R.eye_ray_barycentrics(np.linalg.inv(vp), np.tile(tri, (4, 1, 1)), ndc)
    np.testing.assert_allclose(b, [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1 / 3, 1 / 3, 1 / 3]], atol=1e-10)
    # ... where the screen-space centroid is somewhere else entirely
    mid = ndc[:3].mean(axis=0, keepdims=True)
    assert np.abs(R.eye_ray_barycentrics(np.linalg.inv(vp), tri[None], mid)[0] - 1 / 3).max() > 0.2


def test_stores_round_as_the_formats_say():
    tab6 = R.ufloat_values(6)
    assert R.ufloat_code(np.array([0.0, -1.0, 1.0, 65024.0, 1e9, tab6[1] / 2, np.nextafter(tab6[1] / 2, 1.0)]), 6).tolist() == [0, 0, 15 << 6, 1983, 1983, 0, 1]
    mid = 0.5 * (tab6[100] + tab6[101]), 0.5 * (tab6[101] + tab6[102])
    assert R.ufloat_code(np.array(mid), 6).tolist() == [100, 102]      # ties to even
    assert R.unorm_code(np.array([0.5, -0.1, 2.0, 0.5 / 255 - 1e-9]), 255).tolist() == [128, 0, 255, 0]
    o = O.Oracle(4, 4)
    try:
        rng = np.random.default_rng(0)
        x = np.concatenate([10.0 ** rng.uniform(-8, 5, 2000), tab6[:200], 0.5 * (tab6[:200] + tab6[1:201])])
        for v in x:
            w = int(o.L.orc_pack_r11g11b10f(np.array([v, v, v], np.float32).ctypes.data_as(O.C.c_void_p)))
            f = float(np.float32(v))
            assert (w & 0x7FF, w >> 22) == (int(R.ufloat_code(f, 6)), int(R.ufloat_code(f, 5))), v
    finally:
        o.close()
