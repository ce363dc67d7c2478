"""The float64 model of paths of D levels and N samples per pixel (tests/shading_ref.py: follow_paths, frame(depth, samples)) on the CPU, no
GPU.  The model is written from the rule texts of rtggx_set_max_recursion_depth and rtggx_set_samples_per_pixel in include/rtggx.h and is
no port of the restatements (tests/recursion_ref.cpp, tests/spp_ref.cpp) it is compared with.

  a  frame(depth=1, samples=1) is the depth-1 model, every array equal to its statement without a follower (_depth1_images below);
  b  known answers no implementation is witness of: the furnace chain (a constant cube: only the hit sequence comes from geometry), the
     N-sample value as the mean of the model's own N one-sample frames;
  c  every run of shading_cases.path_cases() against the CPU restatement's fp32 values in front of the packs
     (restatement.Oracle(depth=D, samples=N, entry="spp").ray_trace_primary_f32()): the procedure of tests/test_shading_ref_host.py measure --
     the patterns, the ray count within 2 x flagged pixels x N x D, THE FLOOR in fp32 ulps of the pixel's largest channel on unflagged
     pixels, recorded per run in tests/golden/shading_paths_floor.json and re-measured by every run of this module under FLOOR_DRIFT --
     and the code rule (check_words) on the restatement's words, delta = the run's own recorded maximum x MARGIN; the G-buffer's and the
     velocity's delta stay those of the case's family in the depth-1 file (they do not depend on D or N);
  d  at most FLAG_CAP of a frame's covered pixels are flagged, in every frame of every run: a pixel is flagged if any segment of either
     path of any sample is;
  e  from the model's bookkeeping, over all runs: every way a path can end occurs at a level >= 1 in 100 pixel-frames, both group switches
     and the diffuse group's (1 - m) with 0 < m < 0.5 occur 100 times;
  f  the sun's and the lights' terms at the surfaces the paths hit (shading_ref.hits_pass; shading_cases.hit_cases()), judged through the
     words: the restatement that carries both switches is run with the primary passes left out, switches off, then on; the model adds
     its sum S to the unpacked "off" word and the code rule is asked of the "on" word (check_hit_stage), delta from the same scene's
     recorded path floor; a word without a term stays bit for bit; per kind the walled court supplies 100 terms of each lobe on each
     kind of ray at levels 0 and 1 and occluded, facing-away, out-of-range and outside-the-cone hits; a lit hit worked out by hand.

tests/test_gpu_shading_paths.py runs the same runs on the device.  Regenerate the floor by hand after a deliberate change of the model,
the restatements or the runs (the `gpu_measured` entry is kept):

    python -c "import sys; sys.path[:0] = ['tests', '.']; import test_shading_paths_host as t; t.write_floor()"
"""
import json
import os

import numpy as np
import pytest

import light_hit_ref as LH
import restatement as RS
import sun_ref as SR
import shading_cases as SC
import shading_ref as R
import test_shading_ref_host as HOST
from test_shading_ref_host import FLAG_CAP, FLOOR_DRIFT, GRAZING_NOL_ERROR, MARGIN, ROUGH_CLASS

FLOOR_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_paths_floor.json")
MIN_BRANCH = 100
ENDS = ("miss", "preset", "nol", "last_mirror", "last_diffuse")


# ---- running a run -------------------------------------------------------------------------------------------------------------------
def run_restatement(run, lib=None):
    """Every frame of a run on the restatement -> per frame the words, the rays and (own library only) the fp32 values in front of the packs."""
    case = run.case
    o = RS.Oracle(case.W, case.H, threads=4, depth=run.depth, samples=run.samples, entry="spp") if lib is None else _MutantOracle(case.W, case.H, run.depth, run.samples, lib)
    try:
        HOST.load_oracle(o, case)
        o.build_as(); o.transform_sh()
        out = []
        for k in run.positions:
            o.set_frame_constants(case.constants(k)); o.update_as(); o.render_visibility()
            if lib is None:
                rays, refl, diff, primary = o.ray_trace_primary_f32()
                out.append(dict(HOST.oracle_words(o), rays=rays, refl_f32=refl, diff_f32=diff, primary_f32=primary))
            else:
                rays = o.ray_trace()
                out.append(dict(HOST.oracle_words(o), rays=rays))
        return out
    finally:
        o.close()


class _MutantOracle(RS.Oracle):
    """restatement.Oracle on another build of its library (tests/shading_mutations.py)."""

    def __init__(self, width, height, depth, samples, lib):
        self.depth, self.samples, self.sample_set = depth, samples, 256
        self.entry, self.taken = RS.ENTRIES["spp"]
        RS.O.Oracle.__init__(self, width, height, 4, lib=lib)


_MODEL = {}


def model_frames(run, vis_per_frame):
    """The model's frames of a run, computed once per process for the visibility words given."""
    if run.name not in _MODEL:
        case = run.case
        scene, prev, frames = R.Scene(case.meshes, case.cube), None, []
        for k, vis in zip(run.positions, vis_per_frame):
            prev = R.frame(scene, case.constants(k), vis, case.W, case.H, case.vndf, prev, depth=run.depth, samples=run.samples)
            prev["vis"] = np.array(vis)
            frames.append(prev)
        _MODEL[run.name] = frames
    for m, vis in zip(_MODEL[run.name], vis_per_frame):
        np.testing.assert_array_equal(m["vis"], vis, err_msg="%s: the visibility words differ from those the model was run on" % run.name)
    return _MODEL[run.name]


def recorded():
    return json.load(open(FLOOR_PATH))


def bounds_of(run, rec=None):
    """What check_words takes: the run's own recorded floor for the two images, the family's depth-1 floor for the G-buffer and the velocity."""
    rec = rec or recorded()
    fam = HOST.recorded()["bounds"][run.case.family]
    return {"refl": rec["runs"][run.name]["refl"], "diff": rec["runs"][run.name]["diff"], "gbuffer": fam["gbuffer"], "velocity": fam["velocity"]}


def branch_counts(m):
    """Of one frame: how the paths ended at a level >= 1, by kind (pixel-frames: a pixel counts once per kind and frame), and the events."""
    out = {}
    for code, name in R.TERM_NAMES.items():
        deep = ((m["refl_term"] == code) & (m["refl_term_level"] >= 1)) | ((m["diff_term"] == code) & (m["diff_term_level"] >= 1))
        out[name] = int(deep.any(axis=0).sum())
    out.update({e: int(v) for e, v in m["events"].items()})
    return out


# ---- c, d: a run against the restatement's fp32 values ---------------------------------------------------------------------------------
def measure(run, floor=None):
    """Asserts c's patterns and d on every frame; returns the run's entry of the floor table."""
    case = run.case
    frames = run_restatement(run)
    models = model_frames(run, [f["vis"] for f in frames])
    e, rough_e = {"refl": [], "diff": []}, {"refl": [], "diff": []}
    flags_seen, shares, branches, grazing, rays_levels = 0, [], {}, 0, np.zeros(run.depth, np.int64)
    for k, f, m in zip(run.positions, frames, models):
        label = "%s frame %d" % (run.name, SC.FRAMES[k])
        ok, cov = m["flags"] == 0, m["covered"]
        share = HOST.flagged_share(m)
        shares.append(share)
        assert share <= FLAG_CAP, "%s: %.2f %% of the covered pixels are flagged (%s): change the run, not the cap" % (
            label, 100 * share, {n: int(((m["flags"] & b) != 0).sum()) for b, n in R.FLAG_NAMES.items()})
        flags_seen |= int(np.bitwise_or.reduce(m["flags"].reshape(-1)))
        n_flagged = int((~ok).sum())
        assert abs(f["rays"] - m["rays"]) <= 2 * n_flagged * run.samples * run.depth, "%s: %d rays, the model traces %d (%d pixels flagged)" % (label, f["rays"], m["rays"], n_flagged)
        untraced = ok & cov & ~m["refl_traced"]
        assert (f["refl_f32"][untraced] == 0.0).all(), "%s: a value where the model traces no reflection ray" % label
        somewhere = ok & cov & m["refl_traced"] & (np.minimum(np.abs(m["refl_lo"]), np.abs(m["refl_hi"])).max(axis=-1) > 1e-6) & (m["refl_lo"] * m["refl_hi"] > 0).any(axis=-1)
        assert (np.abs(f["refl_f32"][somewhere]).max(axis=-1) > 0.0).all(), "%s: zero where the model's reflection paths bring something back" % label
        assert np.isnan(f["diff_f32"][cov & ~m["diff_traced"]]).all() and not np.isnan(f["diff_f32"][ok & m["diff_written"]]).any(), "%s: the diffuse rays' pattern" % label
        for key, where in (("refl", ok), ("diff", ok & m["diff_written"])):
            assert np.isfinite(f[key + "_f32"][where]).all() and np.isfinite(m[key + "_lo"][where]).all() and np.isfinite(m[key + "_hi"][where]).all(), "%s: non-finite %s" % (label, key)
            e[key].append(R.ulp_distance(f[key + "_f32"][where], m[key + "_lo"][where], m[key + "_hi"][where]))
            rough_e[key].append(e[key][-1][((m["rm_value"][..., 0] >= ROUGH_CLASS) | ~cov)[where]])
        # level 0's grazing reflections, as in the depth-1 test: each grazing sample's value is C NoL, so the sum may be off by the samples' C x
        # GRAZING_NOL_ERROR / N (refl_graze) and the well-conditioned pixels' floor
        gz = (m["flags"] == R.FLAG_GRAZING) & cov
        if gz.any() and floor is not None:
            hi_abs = np.maximum(np.abs(m["refl_lo"][gz]), np.abs(m["refl_hi"][gz])).max(axis=-1)
            dist = np.maximum(np.maximum(m["refl_lo"][gz] - f["refl_f32"][gz], f["refl_f32"][gz] - m["refl_hi"][gz]), 0.0).max(axis=-1)
            allowed = m["refl_graze"][gz] * GRAZING_NOL_ERROR + MARGIN * floor["refl"]["max"] * R.ulp32(hi_abs)
            assert (dist <= allowed).all(), "%s: a grazing reflection is off by %.3g, allowed %.3g" % (label, dist[np.argmax(dist - allowed)], allowed[np.argmax(dist - allowed)])
            grazing += int(gz.sum())
        for name, v in branch_counts(m).items():
            branches[name] = branches.get(name, 0) + v
        rays_levels += m["rays_levels"]
    entry = {key: R.quantiles(np.concatenate(v)) for key, v in e.items()}
    for key, v in rough_e.items():
        entry[key]["max_rough"] = float(np.concatenate(v).max(initial=0.0))
    entry.update(case=case.name, depth=run.depth, samples=run.samples, frames=[SC.FRAMES[k] for k in run.positions], flagged_share=shares,
                 flags_seen=sorted(n for b, n in R.FLAG_NAMES.items() if flags_seen & b), branches=branches, rays_levels=[int(x) for x in rays_levels])
    return entry, frames, models


# What dominates each run's floor (read from the worst unflagged pixels when the floor was first measured).
_CARRIED = ("the hit point P = o + t dir carried into the next level: its fp32 error along the surface is the ray's own over the cosine of incidence, and the next "
            "ray's hit, checkerboard cell and cube direction move with it")
_ROOM = "reflection: the room's checkerboard at roughness codes below 0.05 (the cancelling root of the sampler) met at the first and again at a deeper level; both images: "
_ZERO = ("nothing: the room is black and fully metallic, every path ends at level 1 with the preset (0) or carries the throughput 0, and model and restatement agree on "
         "zero exactly; the run holds the preset rule, the pattern and the ray counts per level")
_OPEN = ("reflection: as the depth-1 floor of the case (the primary surface's barycentrics from screen-space gradients, times the cube's slope); few paths go on: the "
         "second level's hits are the occluder's and the sheets' undersides, most deeper rays miss")
_MEAN = "as the depth-1 floor of the case, sample by sample: the worst sample's error over N (the sum itself adds N - 1 roundings of half an ulp)"
DOMINATES = {
    "materials_0_64x48_d2n1": _ROOM + _CARRIED,
    "materials_1_64x48_d2n1": "reflection: level-0 NoL of 0.009 to 0.03 just above the grazing flag (relative error = absolute error of NoL over NoL), then " + _CARRIED
                              + "; diffuse: two roundings, the room is a diffuse chain",
    "room_2_64x48_d2n1": "both images: a mirror wall (metallic 0.75, roughness 0.35 x 0.25 on the odd cells) seen in a mirror wall: the sampler's root twice, and " + _CARRIED,
    "materials_3_64x48_d2n1": _ZERO, "materials_3_64x48_d3n1": _ZERO, "materials_3_64x48_vndf_d3n1": _ZERO, "materials_3_64x48_d4n1": _ZERO, "materials_3_64x48_vndf_d4n1": _ZERO,
    "materials_3_64x48_d2n2": _ZERO,
    "materials_0_64x48_d3n1": _ROOM + _CARRIED + ", twice",
    "materials_1_64x48_d4n1": "reflection: as materials_1 at depth 2 (the same pixels: level-0 NoL 0.009), three carried hit points; diffuse: a chain of colour products",
    "materials_1_64x48_vndf_d3n1": "reflection: as materials_1 at depth 2 under the VNDF map; diffuse: a chain of colour products",
    "materials_0_64x48_vndf_d4n1": "reflection: roughness 0.004 on the checkerboard under the VNDF map (the root of 1 - t1^2 - t2^2), then " + _CARRIED + ", three times; diffuse: "
                                   "hits whose shading normal faces away from the ray (N.V of -0.1 to 0) on the ball's silhouette",
    "materials_1_64x48_d2n2": "as materials_1 at depth 2, the mean of two samples",
    "room_2_64x48_d3n1": "both images: as room_2 at depth 2 with a third mirror bounce; the diffuse image's worst pixels leave the ball at N.V 0.04",
    "sheets_vertex_96x64_d2n1": _OPEN, "skew_75x53_d2n1": _OPEN + "; reflection NoL of 0.1 at roughness 0.16 on the cap", "mirrored_bias_75x53_d2n1": _OPEN,
    "sun_75x53_d2n1": _OPEN + "; reflection: the slab's checkerboard at roughness 0.025", "lights_75x53_d2n1": _OPEN,
    "court_64x48_d1n1": "reflection: NoL of a few 1e-2 on the ball's rim and on the walls seen at grazing angles; both images: the screen-space barycentrics times the cube's slope",
    "court_64x48_d2n1": "as the court at depth 1, then " + _CARRIED + "; half of the second rays leave through the open top",
    "sheets_vertex_96x64_d1n8": _MEAN, "skew_75x53_d1n2": _MEAN,
    "materials_3_64x48_d1n4": "reflection: the ball (roughness 0.8 to 1, metallic 0.75) seen in itself under its interpolated normals (a hit with N.V < 0), and the black room's "
                              "roughness 0.013 to 0.04; " + _MEAN,
}


def write_floor():
    runs = {r.name: measure(r)[0] for r in SC.path_cases()}
    doc = {"about": "fp32 ulps (of the pixel's largest channel) by which the CPU restatement's values in front of their packs, at recursion depth D and N samples per "
                    "pixel, differ from the float64 model's interval, unflagged pixels, all frames of a run; written by tests/test_shading_paths_host.py "
                    "write_floor(), re-measured by every run of that module", "margin": MARGIN, "flag_cap": FLAG_CAP, "cancel_slack": R.CANCEL_SLACK,
           "grazing_nol": R.GRAZING_NOL, "runs": runs, "dominates": DOMINATES}
    with open(FLOOR_PATH, "w") as f:      # (the hit runs read their delta from the runs just measured)
        json.dump(dict(doc, hit_runs={}), f, indent=1, sort_keys=True)
    doc["hit_runs"] = {r.name: measure_hits(r)[0] for r in SC.hit_cases()}
    doc["furnace"] = {str(d): furnace_distance(d) for d in (1, 2, 3, 4)}
    if os.path.exists(FLOOR_PATH):
        old = json.load(open(FLOOR_PATH))
        if "gpu_measured" in old:
            doc["gpu_measured"] = old["gpu_measured"]
    with open(FLOOR_PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc


@pytest.mark.parametrize("name", SC.PATH_NAMES)
def test_run_against_the_restatement_and_its_recorded_floor(name):
    run = SC.path_by_name(name)
    rec = recorded()
    assert (rec["cancel_slack"], rec["grazing_nol"], rec["margin"], rec["flag_cap"]) == (R.CANCEL_SLACK, R.GRAZING_NOL, MARGIN, FLAG_CAP)
    want = rec["runs"][name]
    got, frames, models = measure(run, want)
    print("%s: %s" % (name, json.dumps(got)))
    assert (got["case"], got["depth"], got["samples"], got["frames"], got["flags_seen"]) == (want["case"], want["depth"], want["samples"], want["frames"], want["flags_seen"])
    # the bookkeeping is the recorded one (a decision within a flag's band may fall the other way under another libm: a few counts, not a branch)
    for a, b in [(got["branches"][n], want["branches"][n]) for n in want["branches"]] + list(zip(got["rays_levels"], want["rays_levels"])):
        assert abs(a - b) <= 0.01 * b + 5, "%s: the recorded bookkeeping is not this run's: %s %s, recorded %s %s" % (name, got["branches"], got["rays_levels"], want["branches"], want["rays_levels"])
    assert max(got["flagged_share"]) <= FLAG_CAP and max(want["flagged_share"]) <= FLAG_CAP
    for key in ("refl", "diff"):
        assert got[key]["n"] == want[key]["n"], "%s %s: number of compared pixels" % (name, key)
        for q in want[key]:
            if q != "n":      # a measurement: last bits of libm and numpy move it; what is asked is that it has not grown
                assert got[key][q] <= FLOOR_DRIFT * want[key][q] + 0.5, "%s %s %s: the floor grew: %.3f, recorded %.3f" % (name, key, q, got[key][q], want[key][q])
    prev, bounds = None, bounds_of(run, rec)
    for k, f, m in zip(run.positions, frames, models):
        HOST.check_words("%s frame %d" % (name, SC.FRAMES[k]), f, m, prev, bounds)
        prev = f


def test_the_recorded_runs_reach_every_branch():
    rec = recorded()
    assert sorted(rec["runs"]) == sorted(SC.PATH_NAMES) and sorted(rec["dominates"]) == sorted(SC.PATH_NAMES)
    total = {}
    for r in rec["runs"].values():
        assert max(r["flagged_share"]) <= FLAG_CAP
        for name, v in r["branches"].items():
            total[name] = total.get(name, 0) + v
    for name in ENDS + R.EVENTS:
        assert total[name] >= MIN_BRANCH, "%s occurs %d times over all runs: %s" % (name, total[name], total)
    # under each sampler a depth-4 run carries rays at every level (materials_3's do not: see path_cases), and index 255 at eight samples is among the frames
    for vndf in (False, True):
        assert any(min(r["rays_levels"]) > 1000 for n, r in rec["runs"].items() if r["depth"] == 4 and SC.path_by_name(n).case.vndf == vndf)
    assert any(r["samples"] == 8 and 255 in r["frames"] for r in rec["runs"].values())
    assert all(255 in r["frames"] for r in rec["runs"].values() if r["samples"] > 1)


# ---- the sun and the lights at the hits (shading_ref.hits_pass), stage by stage ------------------------------------------------------------
def hit_lights(run, k):
    return HOST.light_dicts(run.lights(k)) if run.lights is not None else []


def hit_sun(run, k):
    if run.sun is None:
        return None
    d, e = run.sun(k)
    return SR.normalise(d), e


def set_hit_lighting(o, run, k, on):
    """The run's sun and lights of frame position k on an oracle or a context (the same method names), the switches of its kind at `on`."""
    if run.sun is not None:
        o.set_sun(*run.sun(k))
    else:
        o.set_sun(None, None)
    o.set_lights(run.lights(k) if run.lights is not None else [])
    o.set_sun_reflections(1 if on and run.sun is not None else 0)
    o.set_light_reflections(1 if on and run.lights is not None else 0)


def run_hit_restatement(run, lib=None):
    """Every frame of a hit run on the restatement that carries both switches (tests/light_hit_ref.py), twice: the switches off, then on.
    -> per frame {"off" / "on": the words IN FRONT OF the primary passes of rtggx_set_sun / rtggx_set_lights (S is added to the packed word there,
    and those passes unpack and pack it again: behind them the stage is no longer one rounding), "rays_off" / "rays_on" of the walk alone}."""
    case = run.case
    own = LH._lib
    if lib is not None:
        LH._lib = lib
    try:
        o = LH.Oracle(case.W, case.H, threads=4, depth=run.depth, samples=1)
    finally:
        LH._lib = own
    try:
        HOST.load_oracle(o, case)
        o.build_as(); o.transform_sh()
        o.force_walker = True
        o.sun_apply = lambda: 0                      # (the primary passes left out: the walk's words as they stand in front of them)
        o.lights_apply = lambda *a, **kw: 0
        out = []
        for k in run.positions:
            o.set_frame_constants(case.constants(k)); o.update_as(); o.render_visibility()
            f = {}
            for name, on in (("off", 0), ("on", 1)):
                set_hit_lighting(o, run, k, on)
                f["rays_" + name] = o.ray_trace()
                f[name] = HOST.oracle_words(o)
            out.append(f)
        return out
    finally:
        o.close()


def check_hit_stage(label, before, after, p, bounds, only=None):
    """The hit sum against the model: the words `after` it from the words `before` it, on unflagged pixels (and `only` [2 H W], where given):
    the code rule where a term exists, the word bit for bit where none does.  -> {image: (allowance used, values compared)}."""
    ok = p["flags"] == 0
    used = {}
    for img, (name, key) in enumerate((("RayTracingOut0", "refl"), ("RayTracingOut1", "diff"))):
        where = ok & p["term"][img] & (only[img] if only is not None else True)
        base = R.unpack_r11g11b10(before[key])
        lo, hi = base + p["lo"][img], base + p["hi"][img]
        delta = bounds[key]["max"] * MARGIN * R.ulp32(np.maximum(np.abs(lo), np.abs(hi)).max(axis=-1))
        stored = R.r11g11b10_split(after[key])
        a_sum = 0
        for ch, mb in enumerate((6, 6, 5)):
            bad, allowance = R.code_rule(lambda x, mb=mb: R.ufloat_code(x, mb), stored[..., ch], lo[..., ch], hi[..., ch], delta)
            at = np.argwhere(bad & where)
            assert at.size == 0, "%s: %s channel %d breaks the code rule at %d values, first (y, x) %s: stored code %s, the model's value in [%s, %s]" % (
                label, name, ch, len(at), at[0].tolist(), stored[..., ch][tuple(at[0])], lo[..., ch][tuple(at[0])], hi[..., ch][tuple(at[0])])
            a_sum += int((allowance & where).sum())
        used[name] = (a_sum, 3 * int(where.sum()))
        still = ok & ~p["term"][img] & (only[img] if only is not None else True)
        np.testing.assert_array_equal(after[key][still], before[key][still], err_msg="%s: %s changed where no term exists" % (label, name))
    return used


def hit_bounds(run, rec=None):
    """The stage's delta: the floor the same scene's paths record at the run's depth (a depth-1 case of the depth-1 file: that file's)."""
    rec = rec or recorded()
    name = "%s_d%dn1" % (run.case.name, run.depth)
    return rec["runs"][name] if name in rec["runs"] else HOST.recorded()["cases"][run.case.name]


_HIT_MODEL = {}


def hit_models(run, vis_per_frame):
    """Per frame (the model's frame at the run's depth, its hits_pass), once per process."""
    if run.name not in _HIT_MODEL:
        case = run.case
        frames = model_frames(SC.PathRun(case, run.depth, 1), vis_per_frame)
        scene = R.Scene(case.meshes, case.cube)
        _HIT_MODEL[run.name] = [(m, R.hits_pass(scene, case.constants(k), m, hit_sun(run, k), hit_lights(run, k))) for k, m in zip(run.positions, frames)]
    return _HIT_MODEL[run.name]


def measure_hits(run, frames=None, bounds=None):
    """The stage check on every frame of a hit run (the restatement's words in front of the primary passes, or `frames`) and the run's
    bookkeeping: flag shares, terms by level and lobe, hits by class."""
    frames = frames or run_hit_restatement(run)
    bounds = bounds or hit_bounds(run)
    counts, shares, used, lights_max = {}, [], {}, 0
    for k, f, (m, p) in zip(run.positions, frames, hit_models(run, [f["off"]["vis"] for f in frames])):
        label = "%s frame %d" % (run.name, SC.FRAMES[k])
        share = float(((p["flags"] != 0) & m["covered"]).sum()) / max(int(m["covered"].sum()), 1)
        shares.append(share)
        assert share <= FLAG_CAP, "%s: %.2f %% of the covered pixels flagged" % (label, 100 * share)
        n_lights = len(hit_lights(run, k)) + (run.sun is not None)
        flagged = int((p["flags"] != 0).sum())
        if "rays_on" in f:
            assert abs((f["rays_on"] - f["rays_off"]) - p["rays"]) <= 2 * n_lights * flagged * run.depth, "%s: %d shadow rays from hits, the model %d" % (
                label, f["rays_on"] - f["rays_off"], p["rays"])
        for img, (a, b) in check_hit_stage(label, f["off"], f["on"], p, bounds, f.get("only")).items():
            t = used.setdefault(img, [0, 0]); t[0] += a; t[1] += b
        for (lev, name), v in p["counts"].items():
            counts["level %d %s" % (lev, name)] = counts.get("level %d %s" % (lev, name), 0) + v
    return {"case": run.case.name, "depth": run.depth, "kind": run.kind, "flagged_share": shares, "counts": counts, "compared": {k: v[1] for k, v in used.items()}}, used


@pytest.mark.parametrize("name", SC.HIT_NAMES)
def test_sun_and_lights_at_the_hits_against_the_model(name):
    run = SC.hit_by_name(name)
    got, used = measure_hits(run)
    print("%s: %s %s" % (name, json.dumps(got), used))
    want = recorded()["hit_runs"][name]
    assert (got["case"], got["depth"], got["kind"]) == (want["case"], want["depth"], want["kind"]) and max(got["flagged_share"]) <= FLAG_CAP
    for key, v in want["counts"].items():
        assert abs(got["counts"].get(key, 0) - v) <= 0.01 * v + 5, "%s: %s: %s, recorded %s" % (name, key, got["counts"].get(key, 0), v)
    assert all(v > 0 for v in got["compared"].values())


def test_the_recorded_hit_runs_reach_every_class():
    rec = recorded()["hit_runs"]
    assert sorted(rec) == sorted(SC.HIT_NAMES)
    for kind in ("sun", "lights", "both"):      # per kind, on the walled court (the open scenes supply a few terms at level 1 and next to no diffuse lobe)
        c = rec["court_64x48_d2_%s_hits" % kind]["counts"]
        for lev in (0, 1):
            for lobe in R.LOBES:
                assert c.get("level %d %s" % (lev, lobe), 0) >= MIN_BRANCH, "%s: level %d %s: %s" % (kind, lev, lobe, c)
        classes = ("facing_away", "occluded") + (("out_of_range", "outside_cone") if kind != "sun" else ())
        for cls in classes:
            assert sum(c.get("level %d %s" % (lev, cls), 0) for lev in (0, 1)) >= 20, "%s: %s: %s" % (kind, cls, c)
    for r in rec.values():
        assert max(r["flagged_share"]) <= FLAG_CAP


# ---- a: the defaults are the depth-1 model -----------------------------------------------------------------------------------------------
def _depth1_images(scene, fc_bytes, m, W, H, vndf):
    """The two images of a depth-1, one-sample frame stated without a follower: per covered pixel the level-0 ray (the primary surface is
    taken from m) meets the scene once and the hit is shaded as the last level.  -> (refl_lo, refl_hi, diff_lo, diff_hi) at covered pixels."""
    fc = R.read_constants(fc_bytes)
    s = m["surface"]
    geo = R._world_triangles(scene, fc)
    c = np.nonzero(s["covered"])[0]
    slot, xi = R.sample_params(W, H, fc["frame_index"])
    phi = 2.0 * np.pi * slot / 256.0
    out = []
    for image in (0, 1):
        runs = []
        for slack in (0.0, -R.CANCEL_SLACK, R.CANCEL_SLACK):
            lo, hi = np.zeros((c.size, 3)), np.zeros((c.size, 3))
            if image == 0:
                al = s["rough"][c] ** 2
                Hh = (R.vndf_half_vector(s["N"][c], s["V"][c], al, phi[c], xi[c], slack) if vndf else R.ndf_half_vector(s["N"][c], al, phi[c], xi[c], slack))[0]
                d = 2.0 * R._dot(s["V"][c], Hh)[:, None] * Hh - s["V"][c]
                NoL = R._dot(s["N"][c], d)
                f0 = R.f0_of(s["colour"][c], s["metal"][c])
                VoH, NoH, NoV = R._sat(R._dot(s["V"][c], Hh)), R._sat(R._dot(s["N"][c], Hh)), R._sat(R._dot(s["N"][c], s["V"][c]))
                w = R.vndf_weight(f0, al, NoL, VoH) if vndf else R.ndf_weight(f0, al, NoV, NoL, VoH, NoH)
                go = NoL > 0.0
            else:
                d = R.sphere_direction(s["N"][c], phi[c], xi[c], slack)
                w = s["colour"][c] * 0.96
                go = s["metal"][c] < 1.0
            g = np.nonzero(go)[0]
            h = R.closest_hit(geo[0], s["P"][c][g], d[g], s["tri_of"][c][g])
            preset = (s["colour"][c] * s["metal"][c][:, None])[g]
            miss = ~h["valid"]
            dark = h["valid"] & (preset <= 0.0).all(axis=1) & (image == 0)
            l, u = np.zeros((g.size, 3)), np.zeros((g.size, 3))
            if miss.any():
                l[miss], u[miss] = scene.environment(d[g][miss], 0.0)
            l[dark] = u[dark] = preset[dark]
            k = np.nonzero(h["valid"] & ~dark)[0]
            if k.size:
                a = R._attributes(scene, fc, geo[1][h["tri"][k]], geo[2][h["tri"][k]], h["b"][k])
                l[k], u[k], _ = R._last_level(scene, a, d[g][k], np.full(k.size, image == 1))
            lo[g], hi[g] = R._scale(l, u, w[g])
            runs.append((lo, hi))
        out += [np.minimum.reduce([r[0] for r in runs]), np.maximum.reduce([r[1] for r in runs])]
    return out


@pytest.mark.parametrize("name", ["skew_75x53", "materials_3_64x48_vndf"])
def test_the_defaults_are_the_depth_1_model(name):
    case = SC.by_name(name)
    frames = HOST.run_oracle(case)
    scene, prev, prev_d = R.Scene(case.meshes, case.cube), None, None
    for k, f in enumerate(frames):
        m = R.frame(scene, case.constants(k), f["vis"], case.W, case.H, case.vndf, prev)
        explicit = R.frame(scene, case.constants(k), f["vis"], case.W, case.H, case.vndf, prev_d, depth=1, samples=1)
        for key, v in m.items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(v, explicit[key], err_msg="%s frame %d: %s" % (name, k, key))
        assert m["rays"] == explicit["rays"] == int(m["refl_traced"].sum() + m["diff_traced"].sum()) and m["rays_levels"].tolist() == [m["rays"]]
        c = m["covered"]
        rl, rh, dl, dh = _depth1_images(scene, case.constants(k), m, case.W, case.H, case.vndf)
        np.testing.assert_array_equal(m["refl_lo"][c], rl); np.testing.assert_array_equal(m["refl_hi"][c], rh)
        w = (m["diff_traced"])[c]
        np.testing.assert_array_equal(m["diff_lo"][c][w], dl[w]); np.testing.assert_array_equal(m["diff_hi"][c][w], dh[w])
        assert ((m["refl_term_level"] == 0) & (m["diff_term_level"] == 0)).all()
        prev, prev_d = m, explicit


# ---- b: known answers ------------------------------------------------------------------------------------------------------------------
def furnace_run():
    """The closed room around the ball under the constant cube, both instances non-metallic with m in (0, 0.5)."""
    base = SC.by_name("materials_2_64x48")
    a, b, ma, mb = (0.8, 0.5, 0.3), (0.4, 0.9, 0.6), 0.125, 0.375
    case = SC.Case("furnace_64x48", "materials", 64, 48, SC.room(), SC.closed_ball(), base.world0, base.world1, base.eye, base.focus, SC.constant_cube(),
                   SC._fixed((a, 0.4, ma), (b, 0.6, mb)), eye_step=base.eye_step)
    return case, np.array([a, b], np.float32).astype(np.float64), np.array([ma, mb])      # (the colours as the constants hold them)


def furnace_distance(depth):
    """A constant cube of radiance L in a closed room of diffuse surfaces: the diffuse image at depth D is L 0.96 c_0 prod_{d=1..D} c'_d with
    c'_d = colour (1 - m) of the instance hit at level d - 1: 0.96 once, (1 - m) at every deeper level, the product forward.  Only the hit
    sequence comes from geometry (the model's segments).  The model to 1e-12 relative -- with the model's own projected irradiance / pi at
    the last normal in L's place, so that factor is the model against itself; that it is L is held beside it, to the 1e-6 the projection's
    quadrature gives.  -> the restatement's largest distance from the paper value on unflagged pixels, in fp32 ulps (the furnace's own floor)."""
    case, colour, metal = furnace_run()
    run = SC.PathRun(case, depth, 1, (0,))
    f = run_restatement(run)[0]
    m = model_frames(run, [f["vis"]])[0]
    L = 1.5
    n = case.W * case.H
    inst0 = np.minimum((np.where(f["vis"] > 0, f["vis"].astype(np.int64) - 1, 0) >> 24).reshape(-1), 1)
    want = L * 0.96 * colour[inst0]
    seen = np.zeros(n, np.int64)
    geo_inst = np.concatenate([np.full(len(i.reshape(-1, 3)), k) for k, (_, i) in enumerate(case.meshes)])
    scene = R.Scene(case.meshes, case.cube)
    for sg in sorted((s for s in m["segments"] if s["image"] == 1 and s["run"] == 0), key=lambda s: s["level"]):
        hit = geo_inst[sg["tri_of"]]
        want[sg["path"]] *= (colour[hit] * (1.0 - metal[hit])[:, None])
        seen[sg["path"]] += 1
        if sg["level"] + 1 == depth:      # the radiance the chain ends with: the projected cube's irradiance / pi at the last normal, which is L to the
            e = R.sh_irradiance(scene.sh, sg["N"]) / np.pi      # accuracy of the projection's quadrature over the texels (1e-7), not to 1e-12
            np.testing.assert_allclose(e, L, rtol=1e-6)
            want[sg["path"]] *= e / L
    cov = m["covered"].reshape(-1)
    assert (seen[cov] == depth).all(), "a closed room: every diffuse path runs to the last level"
    got_lo, got_hi = m["diff_lo"].reshape(n, 3)[cov], m["diff_hi"].reshape(n, 3)[cov]
    np.testing.assert_allclose(got_lo, want[cov], rtol=1e-12, atol=0); np.testing.assert_allclose(got_hi, want[cov], rtol=1e-12, atol=0)
    ok = cov & (m["flags"].reshape(-1) == 0)
    assert ok.sum() > 0.9 * cov.sum()
    return float(R.ulp_distance(f["diff_f32"].reshape(n, 3)[ok], want[ok], want[ok]).max())


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_furnace_chain(depth):
    """The restatement's fp32 furnace against the paper value, held to the furnace's own recorded floor: a chain of D + 1 products and the SH
    sum, a few ulps."""
    got, floor = furnace_distance(depth), recorded()["furnace"][str(depth)]
    print("furnace depth %d: %.2f ulps, recorded %.2f" % (depth, got, floor))
    assert floor <= 8.0 * (depth + 2), "the recorded furnace floor is not a few ulps per product: %s" % floor
    assert got <= FLOOR_DRIFT * floor + 0.5, "the restatement's furnace is %.1f ulps off, recorded %.1f" % (got, floor)


def test_a_lit_hit_by_hand():
    """A mirror (roughness 0, metallic 1: H = N, the weight w0 = F) under a diffuse quad that faces a zenith sun: the pixel's reflection ray
    meets the quad from below, and the term the sun adds to RayTracingOut0 is w0 colour (NoL / pi) E with NoL = 1 -- no 0.96, no (1 - m) on a
    reflection-group ray.  V and with it w0 = F0 + (1 - F0)(1 - NoV)^5 come from the pixel's eye ray met with the plane y = 0, worked out here."""
    c0, c1, E = (0.9, 0.6, 0.3), (0.5, 0.25, 0.75), np.array([3.0, 2.0, 1.0])
    eye, focus = (0.0, 2.0, -4.0), (0.0, 0.0, 0.0)
    case = SC.Case("lit_hit_48x32", "hits", 48, 32, SC.grid(1, 1, -3.0, 3.0, -3.0, 3.0), SC.grid(1, 1, -6.0, 6.0, 0.0, 12.0, y=3.0), np.eye(4), np.eye(4), eye, focus,
                   SC.constant_cube(), SC._fixed((c0, 0.0, 1.0), (c1, 0.5, 0.0)), eye_step=(0.0, 0.0, 0.0))
    run = SC.HitRun(case, 1, "sun", sun=lambda k: ((0.0, 1.0, 0.0), tuple(E)))
    run.positions = (0,)
    f = run_hit_restatement(run)[0]
    m, p = hit_models(run, [f["off"]["vis"]])[0]
    y, x = 20, 24
    assert f["off"]["vis"][y, x] == 1 and p["flags"][y, x] == 0 and p["term"][0, y, x] and not p["term"][1, y, x]      # instance 0, triangle 0; metallic 1: no diffuse path
    ndc = np.array([(x + 0.5) / 48 * 2 - 1, -((y + 0.5) / 32 * 2 - 1)])
    fc = R.read_constants(case.constants(0))      # (the matrix and the eye as the constants hold them, in fp32)
    inv, eye = fc["proj_to_world"], fc["eye"]
    a, b = [np.append(ndc, [z, 1.0]) @ inv for z in (0.0, 1.0)]
    a, b = a[:3] / a[3], b[:3] / b[3]
    P = a + (b - a) * (-a[1] / (b[1] - a[1]))
    V = (np.array(eye) - P) / np.linalg.norm(np.array(eye) - P)
    refl = np.array([-V[0], V[1], -V[2]])
    t = 3.0 / refl[1]
    hit = P + t * refl
    assert -6 < hit[0] < 6 and 0 < hit[2] < 12, "the reflection ray meets the quad"
    f0 = np.float32(c0).astype(np.float64)
    w0 = f0 + (1.0 - f0) * (1.0 - V[1]) ** 5
    want = w0 * np.float32(c1).astype(np.float64) * (1.0 / np.pi) * E
    np.testing.assert_allclose(p["mid"][0, y, x], want, rtol=1e-12)
    assert (p["lo"][0, y, x] <= want).all() and (want <= p["hi"][0, y, x]).all() and (p["hi"][0, y, x] - p["lo"][0, y, x] <= 2e-3 * want).all()
    # ... and the restatement's word carries it: the frame in front of the sun's own pass, the switch off, then on
    check_hit_stage("a lit hit by hand", f["off"], f["on"], p, HOST.recorded()["cases"]["sheets_vertex_96x64"])


def test_n_samples_are_the_mean_of_n_one_sample_frames():
    """The model's N-sample value equals the mean of its own N one-sample frames at the indices F N .. F N + N - 1 (exact up to the order
    of the sum), at F = 255 and N = 8: indices 2040 to 2047, not wrapped."""
    case = SC.by_name("sheets_vertex_96x64")
    vis = HOST.run_oracle(case)[2]["vis"]
    scene = R.Scene(case.meshes, case.cube)
    fc = np.frombuffer(case.constants(2), np.uint32).copy()
    assert fc[111] == 255
    many = R.frame(scene, fc.tobytes(), vis, case.W, case.H, depth=2, samples=8)
    lo, hi, rays = 0.0, 0.0, 0
    for k in range(8):
        one = fc.copy(); one[111] = 255 * 8 + k
        m = R.frame(scene, one.tobytes(), vis, case.W, case.H, depth=2, samples=1)
        lo, hi, rays = lo + m["refl_lo"], hi + m["refl_hi"], rays + m["rays"]
        assert (m["refl_term"][0] == many["refl_term"][k]).all() and (m["diff_term_level"][0] == many["diff_term_level"][k]).all()
    c = many["covered"]
    np.testing.assert_allclose(many["refl_lo"][c], lo[c] / 8, rtol=1e-13, atol=1e-300); np.testing.assert_allclose(many["refl_hi"][c], hi[c] / 8, rtol=1e-13, atol=1e-300)
    assert many["rays"] == rays
    assert (R.sample_params(8, 8, 2047)[0] != R.sample_params(8, 8, 2047 & 255)[0]).any(), "a wrapped index draws the same samples"
