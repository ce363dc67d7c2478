"""The sampled lights of the float64 shading model (tests/shading_ref.py: sun_pass with an angle, lights_pass with radii, pick_pass,
records_pass, list_pass and cull_counts, hits_pass with sampled targets) on the CPU, no GPU -- the second witness of rtggx_set_sun_angle,
RtggxLight.radius, rtggx_set_light_sampling(ctx, 1), rtggx_set_light_pick_visibility and rtggx_set_light_list, written from the rule texts of
include/rtggx.h and from nothing else:

  a  known answers neither the kernels nor their restatements are witness of: the disk map's density (uniform in solid angle over the cap,
     every direction inside it), the sphere map's first and second moments over the full enumeration of the draw, the lit share of a
     penumbra against the cap's cut by the edge's plane, the pick's expectation from the integer measure of the draws, the update rule's
     fixed points, the slot sets' disjointness;
  b  the model against the restatements, pass by pass, on shading_cases.sampled_cases(): the words in front of the pass (the restatement's,
     taken as input), the words behind it, the code rule of test_shading_ref_host.check_direct_stage on unflagged pixels, the words bit for
     bit where the model adds nothing, the ray's outcome class per pixel (and per light), the chosen light per pixel, the shadow-ray count;
  c  the cases reach what they were built for (REACH), counted on the model alone, and flag at most FLAG_CAP of the covered pixels per pass;
  d  the floor: the pick's fp32 terms S0, S1 (the restatement exposes them) against the model's intervals in fp32 ulps, recorded in
     tests/golden/shading_sampled_floor.json and re-measured by every run; the disk's and the radii's terms are the directional sun's and the
     radius-0 lights' bit for bit (only visibility is sampled), so their delta is the one those passes are held to: the floor the same
     scenes' ray-traced path records in tests/golden/shading_synthetic_floor.json.

Regenerate the floor by hand after a deliberate change of the model, the restatements or the cases (the `gpu_measured` entry is kept):

    python -c "import sys; sys.path[:0] = ['tests', '.']; import test_shading_sampled_host as t; t.write_floor()"

  e  the visibility records (rtggx_set_light_pick_visibility), one frame at a time (measure_records): the image read and the frame's velocity
     and normal words in, the whole record out -- eight bytes, normal word, stamp --, exact; s and s0 from the call history;
  f  the culled list (rtggx_set_light_list): mode 1's walk over all n lights with the list's slots, and the kept lights per 8 x 8 block
     within the model's [certain, certain + uncertain] (shading_ref.cull_counts);
  g  the sampled targets at the hits (shading_ref.hits_pass with an angle, radii, mode 1 and the list's slots), by the hit stage's check of
     tests/test_shading_paths_host.py, on the court at depth 2."""
import json
import os

import numpy as np
import pytest

import light_list_ref as LL
import light_pick_ref as LP
import lights_ref as LR
import shading_cases as SC
import shading_ref as R
import sun_ref as SR
import sun_soft_ref as SS
import test_shading_ref_host as HOST

FLOOR_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_sampled_floor.json")
FLAG_CAP, MARGIN, FLOOR_DRIFT = HOST.FLAG_CAP, HOST.MARGIN, HOST.FLOOR_DRIFT
DELTA_FROM = {"sun_disk": "sun", "radii": "lights"}      # family -> the family of shading_synthetic_floor.json whose bounds are its delta
# conditions, not measurements: what a case must reach, counted on the model's unflagged pixel-frames
REACH = {"sampled_occluded_centre_lit": 100, "sampled_lit_centre_occluded": 100, "below_horizon": 20,
         "two_candidates": 100, "chosen_each": 20, "later": 20}


# ---- running a case -------------------------------------------------------------------------------------------------------------------
def run_restatement(run):
    """Every frame of a run on the restatement that carries every setting (tests/light_list_ref.py), pass by pass -> per frame
    [("base", words, rays, {}), (label, words, rays, what the restatement tells of the pass), ...]: every pass on the base frame's words."""
    from oracle import oracle as O
    case = run.case
    o = LL.Oracle(case.W, case.H, threads=4)
    try:
        HOST.load_oracle(o, case)
        o.build_as(); o.transform_sh()
        out = []
        for k in run.positions:
            o.set_frame_constants(case.constants(k)); o.update_as(); o.render_visibility()
            o.set_sun(None, None); o.set_lights([]); o.set_light_list([]); o.set_sun_angle(0.0); o.set_light_sampling(0)
            rays = o.ray_trace()
            base = HOST.oracle_words(o)
            stages = [("base", base, rays, {})]
            for label, angle in run.passes(k):
                o.buffer(O.BUF_RT_REFL, copy=False)[...], o.buffer(O.BUF_RT_DIFF, copy=False)[...] = base["refl"], base["diff"]
                if run.kind == "sun":
                    o.set_sun(*case.sun(k)); o.set_sun_angle(angle)
                    rays = o.sun_apply()
                    told = {"classes": o.classes.copy()}
                elif run.kind == "list":
                    o.set_light_list(run.lights(k))
                    rays = o.lights_apply()
                    told = {"info": o.list_info.copy(), "wf": o.list_wf.copy(), "terms": o.list_terms.copy(), "kept": o.list_kept.copy()}
                else:
                    o.set_lights(run.lights(k)); o.set_light_sampling(1 if run.kind == "pick" else 0)
                    rays = o.lights_apply()
                    told = {"classes": o.light_classes.copy()} if run.kind == "lights" else {
                        "info": o.pick_info.copy(), "wf": o.pick_wf.copy(), "terms": o.pick_terms.copy(), "weights": o.pick_weights.copy()}
                stages.append((label, HOST.oracle_words(o), rays, told))
            out.append(stages)
        return out
    finally:
        o.close()


def model_pass(run, k, scene, m, angle=None):
    case = run.case
    if run.kind == "sun":
        d, e = case.sun(k)
        return R.sun_pass(scene, case.constants(k), m, SR.normalise(d), e, angle_degrees=angle)
    lights = light_dicts(run.lights(k))
    return {"pick": R.pick_pass, "lights": R.lights_pass, "list": R.list_pass}[run.kind](scene, case.constants(k), m, lights)


def light_dicts(lights):
    """HOST.light_dicts for any number of lights."""
    return [dict(position=f[0:3], range=f[3], intensity=f[4:7], radius=float(f[7]), axis=f[8:11], cos_outer=f[11], cos_inner=f[12]) for f in LL.records(lights)]


def bounds_of(run):
    rec = recorded()
    return rec["bounds"][run.family]


# ---- b: one pass against the model ---------------------------------------------------------------------------------------------------
SUN_CLASS = {R.OUTCOME_NO_RAY: SS.BELOW_HORIZON, R.OUTCOME_OCCLUDED: SS.OCCLUDED, R.OUTCOME_LIT: SS.LIT}


def check_outcomes(label, run, p, told, covered):
    """The ray's outcome class per pixel, and the chosen light, on unflagged pixels."""
    ok = (p["flags"] == 0) & covered

    def same(got, want, where, what):
        at = np.argwhere(where & (got != want))
        assert at.size == 0, "%s: %s differs from the model's at %d pixels, first (y, x) %s: %s, the model %s" % (
            label, what, len(at), at[0].tolist(), got[tuple(at[0])], want[tuple(at[0])])

    if run.kind == "sun":
        want = np.full(p["outcome"].shape, SS.FACING_AWAY)
        for a, b in SUN_CLASS.items():
            want[p["outcome"] == a] = b
        same(told["classes"].astype(np.int64), want, ok, "the sun ray's class")
    elif run.kind == "lights":
        for i in range(len(p["outcome"])):
            got, out = told["classes"][i].astype(np.int64), p["outcome"][i]
            want = np.where(out == R.OUTCOME_LIT, LR.LIT, np.where(out == R.OUTCOME_OCCLUDED, LR.OCCLUDED, np.where(p["below"][i], LR.BELOW_HORIZON, LR.OUT_OF_RANGE)))
            same(got, want, ok & (out != R.OUTCOME_NONE), "light %d's ray class" % i)
            none = ok & (out == R.OUTCOME_NONE)
            assert np.isin(got[none], (LR.NOT_COVERED, LR.OUT_OF_RANGE, LR.FACING_AWAY, LR.OUTSIDE_CONE)).all(), "%s: light %d has a ray where the model has no candidate" % (label, i)
    else:
        info = told["info"].astype(np.int64)
        same(np.where(info[..., 1] == (LL.NONE if run.kind == "list" else LP.NONE), -1, info[..., 1]), p["chosen"], ok, "the chosen light")
        same(info[..., 0], p["candidates"], ok, "the number of candidates")
        out = p["outcome"]
        want = np.where(out == R.OUTCOME_LIT, LR.LIT, np.where(out == R.OUTCOME_OCCLUDED, LR.OCCLUDED, np.where(p["below"], LR.BELOW_HORIZON, np.where(out == R.OUTCOME_NO_RAY, LR.OUT_OF_RANGE, 0))))
        same(info[..., 2], want, ok, "the chosen ray's class")


def check_stage(label, run, before, after, p, m, bounds, cull_on=True):
    """Assertions b and the flag cap of one pass -> {image: (allowance used, values compared)}.  cull_on: whether the kept counts come from a
    context that culls (check_cull)."""
    covered = m["covered"]
    share = float(((p["flags"] != 0) & covered).sum()) / max(int(covered.sum()), 1)
    assert share <= FLAG_CAP, "%s: %.2f %% of the covered pixels flagged (%s): change the case, not the cap" % (
        label, 100 * share, {n: int(((p["flags"] & b) != 0).sum()) for b, n in R.FLAG_NAMES.items() if ((p["flags"] & b) != 0).any()})
    n_flagged = int((p["flags"] != 0).sum())
    per_pixel = LR.MAX_LIGHTS if run.kind == "lights" else 1      # (rays a flagged pixel may add or lose)
    assert after[2] is None or abs(after[2] - p["rays"]) <= per_pixel * n_flagged, "%s: %s shadow rays, the model %d (%d pixels flagged)" % (label, after[2], p["rays"], n_flagged)
    if after[3]:
        check_outcomes(label, run, p, after[3], covered)
    if run.kind == "list":
        check_cull(label, p["cull"], after[3]["kept"] if after[3] else None, sum(1 for l in run.lights(0) if max(l["intensity"]) > 0), cull_on)
    return HOST.check_direct_stage(label, before[1], after[1], p, bounds), share


def check_cull(label, cull, kept, casting, cull_on=True):
    """The kept lights per block (the restatement's, or the device's counts) within the model's [certain, certain + uncertain]; with the
    cull off, the number of casting lights in every block that has a covered pixel."""
    certain, uncertain, some = cull
    if kept is None:
        return
    kept = np.asarray(kept).astype(np.int64)
    assert kept.shape == certain.shape and (kept[~some] == 0).all(), "%s: a block without a covered pixel keeps a light" % label
    if not cull_on:
        assert (kept[some] == casting).all(), "%s: with the cull off a covered block reads %s, not the %d casting lights" % (label, sorted(set(kept[some].tolist())), casting)
        return
    bad = np.argwhere((kept < certain) | (kept > certain + uncertain))
    assert bad.size == 0, "%s: %d blocks keep a number of lights outside the model's bounds, first (by, bx) %s: %d, the model [%d, %d]" % (
        label, len(bad), bad[0].tolist(), kept[tuple(bad[0])], certain[tuple(bad[0])], (certain + uncertain)[tuple(bad[0])])


def reach_of(run, passes):
    """What the run reaches, counted on the model's unflagged pixel-frames (REACH)."""
    got = dict.fromkeys(("sampled_occluded_centre_lit", "sampled_lit_centre_occluded", "below_horizon", "two_candidates", "later"), 0)
    chosen = {}
    for k, p, m in passes:
        ok = (p["flags"] == 0) & m["covered"]
        out, cen = p["outcome"], p["centre_outcome"]
        got["sampled_occluded_centre_lit"] += int((ok & (out == R.OUTCOME_OCCLUDED) & (cen == R.OUTCOME_LIT)).sum())
        got["sampled_lit_centre_occluded"] += int((ok & (out == R.OUTCOME_LIT) & (cen == R.OUTCOME_OCCLUDED)).sum())
        got["below_horizon"] += int((ok & p["below"]).sum())
        if run.kind == "list":
            certain, uncertain, some = p["cull"]
            casting = sum(1 for l in run.lights(k) if max(l["intensity"]) > 0)
            got["blocks_partly_kept"] = got.get("blocks_partly_kept", 0) + int((some & (uncertain == 0) & (certain > 0) & (certain < casting)).sum())
            got["chosen_from_8"] = got.get("chosen_from_8", 0) + int((ok & (p["chosen"] >= 8)).sum())
            got["chosen_from_64"] = got.get("chosen_from_64", 0) + int((ok & (p["chosen"] >= 64)).sum())
        if run.kind == "pick":
            two = ok & (p["candidates"] >= 2)
            got["two_candidates"] += int(two.sum())
            got["later"] += int((two & p["later"]).sum())
            for i, lt in enumerate(run.lights(k)):
                if max(lt["intensity"]) > 0:
                    chosen["%d:%d" % (k, i)] = int((two & (p["chosen"] == i)).sum())
    if run.kind == "pick":
        got["chosen_each"] = min(chosen.values())
        got["chosen"] = chosen
    return got


def check_reach(run, got):
    if run.kind == "list":
        assert got["blocks_partly_kept"] >= 1 and got["chosen_from_8"] >= 20, "%s: the cull culls nowhere for certain, or no light from 8 on is chosen (%s)" % (run.name, got)
        assert got["below_horizon"] >= REACH["below_horizon"], "%s: the targets' slots decide nothing (%s)" % (run.name, got)
        assert got["chosen_from_64"] >= 1 or len(run.lights(0)) <= 64, "%s: no light of the second chunk is chosen (%s)" % (run.name, got)
        return
    radii = run.kind != "pick" or any(l.get("radius", 0.0) > 0.0 for k in run.positions for l in run.lights(k))
    for name, least in REACH.items():
        if name in ("two_candidates", "chosen_each", "later") and run.kind != "pick":
            continue
        if name in ("sampled_occluded_centre_lit", "sampled_lit_centre_occluded", "below_horizon") and not radii:
            continue      # (a pick without radii samples no visibility: its ray is the centre ray)
        assert got[name] >= least, "%s reaches %s %d times, asked %d: change the case, not the threshold (%s)" % (run.name, name, got[name], least, got)


def measure(run, frames=None, cull_on=True):
    """Every assertion of b and c on a run (the restatement's stages, or the device's) -> its entry of the floor table.  cull_on=False: the
    frames are of a context with rtggx_debug_light_list_cull(ctx, 0), whose kept counts are the casting lights', not the cull rule's."""
    case = run.case
    frames = run_restatement(run) if frames is None else frames
    scene = R.Scene(case.meshes, case.cube)
    models = HOST.model_frames(case, [st[0][1]["vis"] for st in frames])
    bounds = bounds_of(run)
    used, passes, share = {}, [], 0.0
    e = {"refl": [], "diff": []}
    for k, stages, m in zip(run.positions, frames, models):
        for (what, angle), after in zip(run.passes(k), stages[1:]):
            label = "%s frame %d, %s" % (run.name, SC.FRAMES[k], what)
            assert after[0] == what
            p = model_pass(run, k, scene, m, angle)
            if run.kind == "list":
                p["cull"] = R.cull_counts(m, light_dicts(run.lights(k)))
            passes.append((k, p, m))
            u, sh = check_stage(label, run, stages[0], after, p, m, bounds, cull_on)
            share = max(share, sh)
            for img, (a, b) in u.items():
                t = used.setdefault(img, [0, 0]); t[0] += a; t[1] += b
            told = after[3]
            if run.kind in ("pick", "list") and told:      # d: the fp32 terms in front of the add, as the word sees them (on the unpacked word in front of the pass)
                ok = p["flags"] == 0
                S0, S1 = told["terms"][..., :3].astype(np.float64), told["terms"][..., 3:].astype(np.float64)
                assert (S0[ok & ~p["term"]] == 0.0).all() and (S1[ok & ~p["diffuse"]] == 0.0).all(), "%s: a term where the model has none" % label
                for key, S, lo, hi, where in (("refl", S0, p["spec_lo"], p["spec_hi"], ok & p["term"]), ("diff", S1, p["diff_lo"], p["diff_hi"], ok & p["diffuse"])):
                    b0 = R.unpack_r11g11b10(stages[0][1][key])[where]
                    e[key].append(R.ulp_distance(b0 + S[where], b0 + lo[where], b0 + hi[where]))
                one = ok & p["term"] & (p["candidates"] == 1)
                assert (told["wf"][..., 1][one] == 1.0).all(), "%s: f is not exactly 1 with a single candidate" % label
    reach = reach_of(run, passes)
    check_reach(run, reach)
    entry = {"family": run.family, "flagged_share_max": share, "reach": reach, "terms": int(sum(int(p["term"].sum()) for _, p, _ in passes)),
             "rays": int(sum(p["rays"] for _, p, _ in passes))}
    if run.kind in ("pick", "list") and e["refl"]:
        entry.update({key: R.quantiles(np.concatenate(v)) for key, v in e.items()})
    return entry, used


# ---- the visibility records, one frame at a time -----------------------------------------------------------------------------------------
REACH_RECORDS = {"valid_and_carried_below_255": 100, "rejected_each": 20}
_RECORD_MODELS = {}


def record_model_frames(run, vis_per_frame):
    """HOST.model_frames for a record run: frame j at camera position j with its own frame index."""
    case = run.case
    if run.name not in _RECORD_MODELS:
        scene, prev, frames = R.Scene(case.meshes, case.cube), None, []
        for j, vis in enumerate(vis_per_frame):
            prev = R.frame(scene, case.constants(j, run.indices[j]), vis, case.W, case.H, case.vndf, prev)
            prev["vis"] = np.array(vis)
            frames.append(prev)
        _RECORD_MODELS[run.name] = frames
    for m, vis in zip(_RECORD_MODELS[run.name], vis_per_frame):
        np.testing.assert_array_equal(m["vis"], vis, err_msg="%s: the visibility words differ from those the model was run on" % run.name)
    return _RECORD_MODELS[run.name]


def scrambled(read, j):
    """The image frame j reads, overwritten: every byte v random (0, 15, 16 and 255 among them), the left quarter's normals and stamps too."""
    rng = np.random.default_rng(1000 + j)
    out = read.copy()
    out["v"] = rng.integers(0, 256, out["v"].shape).astype(np.uint8)
    out["v"][::3, ::2, :4] = np.array([0, 15, 16, 255], np.uint8)
    q = out.shape[1] // 4
    out["normal"][:, :q] = rng.integers(0, 2 ** 32, (out.shape[0], q), dtype=np.uint64).astype(np.uint32)
    out["stamp"][:, :q] = rng.integers(0, 2 ** 32, (out.shape[0], q), dtype=np.uint64).astype(np.uint32)
    return out


def run_record_restatement(run):
    """Every frame of a record run on the restatement (tests/light_vis_ref.py) beside a twin without lights (the words in front of the pass: a
    successful set_lights is a reset, so the switch cannot be toggled) -> per frame a dict: before, after (words), rays (the pass's), read
    (the image (s - 1) & 1 in front of the pass), old and new (the image s & 1 in front of the frame and behind it), seq, told."""
    import light_vis_ref as LV
    case = run.case
    o, twin = LV.Oracle(case.W, case.H, threads=4), LL.Oracle(case.W, case.H, threads=4)
    try:
        for x in (o, twin):
            HOST.load_oracle(x, case)
            x.build_as(); x.transform_sh()
        o.set_light_sampling(1); o.set_light_pick_visibility(1)
        out = []
        for j, index in enumerate(run.indices):
            if run.lights(j) is not None:
                o.set_lights(run.lights(j))
            for x in (o, twin):
                x.set_frame_constants(case.constants(j, index)); x.update_as(); x.render_visibility()
            base_rays = twin.ray_trace()
            held = o.images.copy()
            read = {}

            def scramble(orc, j=j):
                orc.images[(orc.seq - 1) & 1] = scrambled(orc.images[(orc.seq - 1) & 1], j)
            o.scramble = scramble if j in run.scramble else None
            rays = o.ray_trace()
            s = o.seq
            read = scrambled(held[(s - 1) & 1], j) if j in run.scramble else held[(s - 1) & 1]
            out.append({"before": HOST.oracle_words(twin), "after": HOST.oracle_words(o), "rays": rays - base_rays, "read": read, "old": held[s & 1], "new": o.images[s & 1].copy(),
                        "seq": s, "told": {"info": o.pick_info.copy(), "terms": o.pick_terms.copy(), "wf": o.pick_wf.copy(), "vinfo": o.vis_info.copy()}})
        return out
    finally:
        o.close(); twin.close()


def measure_records(run, frames=None):
    """Every assertion on a record run (the restatement's frames, or the device's), one frame at a time -> its entry of the floor table."""
    case = run.case
    frames = run_record_restatement(run) if frames is None else frames
    scene = R.Scene(case.meshes, case.cube)
    models = record_model_frames(run, [f["after"]["vis"] for f in frames])
    bounds = bounds_of(run)
    seq, lights = R.RecordSequence(), None
    used, e, share = {}, {"refl": [], "diff": []}, 0.0
    reach = {"valid_and_carried_below_255": 0, "rejected": dict.fromkeys(R.HISTORY_NAMES.values(), 0), "updated": 0, "bytes_below_floor": 0}
    terms = rays = 0
    for j, (f, m) in enumerate(zip(frames, models)):
        label = "%s frame %d (index %d)" % (run.name, j, run.indices[j])
        if run.lights(j) is not None:      # a successful rtggx_set_lights: a reset
            lights = light_dicts(run.lights(j))
            seq.reset()
        s, s0 = seq.acting_frame()
        assert f["seq"] == s, "%s: the context's sequence is %d, the rule's %d" % (label, f["seq"], s)
        for key in ("vis", "normal", "rm", "velocity"):
            np.testing.assert_array_equal(f["before"][key], f["after"][key], err_msg="%s: the twin's %s" % (label, key))
        p = R.records_pass(scene, case.constants(j, run.indices[j]), m, lights, f["read"], f["after"]["normal"], f["after"]["velocity"], s, s0)
        cov, ok = m["covered"], (p["flags"] == 0) & m["covered"]
        sh = float(((p["flags"] != 0) & cov).sum()) / max(int(cov.sum()), 1)
        share = max(share, sh)
        assert sh <= FLAG_CAP, "%s: %.2f %% of the covered pixels flagged: change the case, not the cap" % (label, 100 * sh)
        assert f["rays"] is None or abs(f["rays"] - p["rays"]) <= int((p["flags"] != 0).sum()), "%s: %s shadow rays, the model %d" % (label, f["rays"], p["rays"])
        # the twin's words stand for the words in front of the pass only where this frame writes them: RayTracingOut1 under metallic >= 1 is a
        # carry-over of the context's own last frame, lights and all, and the pass never touches it
        kept = ~m["diff_written"]
        if j:
            np.testing.assert_array_equal(f["after"]["diff"][kept], frames[j - 1]["after"]["diff"][kept], err_msg="%s: RayTracingOut1 carried over" % label)
        after = dict(f["after"], diff=np.where(kept, f["before"]["diff"], f["after"]["diff"]))
        for img, (a, b) in HOST.check_direct_stage(label, f["before"], after, p, bounds).items():
            t = used.setdefault(img, [0, 0]); t[0] += a; t[1] += b
        # the records, exactly: what the frame writes at covered pixels, and what it leaves alone
        for field in ("v", "normal", "stamp"):
            got, want = f["new"][field], p["records"][field]
            bad = np.argwhere((got != want).reshape(got.shape[:2] + (-1,)).any(axis=-1) & ok)
            assert bad.size == 0, "%s: the record's %s differs at %d pixels, first (y, x) %s: %s, the model %s (history class %d, chosen %d, outcome %d)" % (
                label, field, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])], p["history"][tuple(bad[0])], p["chosen"][tuple(bad[0])], p["outcome"][tuple(bad[0])])
        assert (f["new"][~cov] == f["old"][~cov]).all(), "%s: a record written where nothing is covered" % label
        told = f["told"]
        if told:
            info = told["info"].astype(np.int64)
            bad = np.argwhere(ok & (np.where(info[..., 1] == LP.NONE, -1, info[..., 1]) != p["chosen"]))
            assert bad.size == 0, "%s: the chosen light differs at %d pixels" % (label, len(bad))
            S0, S1 = told["terms"][..., :3].astype(np.float64), told["terms"][..., 3:].astype(np.float64)
            for key, S, lo, hi, where in (("refl", S0, p["spec_lo"], p["spec_hi"], ok & p["term"]), ("diff", S1, p["diff_lo"], p["diff_hi"], ok & p["diffuse"])):
                b0 = R.unpack_r11g11b10(f["before"][key])[where]
                e[key].append(R.ulp_distance(b0 + S[where], b0 + lo[where], b0 + hi[where]))
        nl = len(lights)
        cands = p["w"] > 0.0      # [nl H W]
        carried = np.moveaxis(p["carried"][..., :nl], -1, 0)
        reach["valid_and_carried_below_255"] += int((ok & (p["history"] == R.HISTORY_VALID) & (cands & (carried != 255)).any(axis=0)).sum())
        reach["bytes_below_floor"] += int((ok & (cands & (carried < R.VIS_FLOOR)).any(axis=0)).sum())
        reach["updated"] += int((ok & ((p["outcome"] == R.OUTCOME_LIT) | (p["outcome"] == R.OUTCOME_OCCLUDED))).sum())
        for cls, name in R.HISTORY_NAMES.items():
            reach["rejected"][name] += int((ok & (p["history"] == cls)).sum())
        terms += int(p["term"].sum()); rays += p["rays"]
    reach["rejected_each"] = min(reach["rejected"].values())
    check_record_reach(run, reach)
    entry = {"family": run.family, "flagged_share_max": share, "reach": reach, "terms": terms, "rays": rays}
    if e["refl"]:
        entry.update({key: R.quantiles(np.concatenate(v)) for key, v in e.items()})
    return entry, used


def check_record_reach(run, got):
    for name, least in REACH_RECORDS.items():
        assert got[name] >= least, "%s reaches %s %d times, asked %d: change the case, not the threshold (%s)" % (run.name, name, got[name], least, got)
    assert got["bytes_below_floor"] >= 20 or not run.scramble, "%s: the floor is applied nowhere (%s)" % (run.name, got)


# ---- the sampled targets at the hits --------------------------------------------------------------------------------------------------------
REACH_HITS = {"terms_level_0": 100, "terms_level_1": 100, "occluded": 100, "below_horizon": 20}


def set_sampled_hit_lighting(x, run, k, on, none=()):
    """The run's settings of frame position k on an oracle or a context (the same method names), the hit switches at `on`.  none: what an
    empty list is for x (a context takes None)."""
    x.set_sun(*(run.sun(k) if run.sun is not None else (None, None)))
    x.set_sun_angle(run.angle)
    x.set_light_sampling(run.mode if not run.as_list else 0)
    lights = run.lights(k) if run.lights is not None else none
    if run.as_list:
        x.set_lights(none); x.set_light_list(lights)
    else:
        x.set_light_list(none); x.set_lights(lights)
    x.set_sun_reflections(1 if on and run.sun is not None else 0)
    x.set_light_reflections(1 if on and run.lights is not None else 0)


def run_sampled_hit_restatement(run):
    """Every frame of a hit run on the restatement (tests/light_list_ref.py), the hit switches off and then on -> per frame {"off" / "on":
    the words IN FRONT OF the primary passes (test_shading_paths_host.run_hit_restatement has the reason), "rays_off" / "rays_on"}."""
    case = run.case
    o = LL.Oracle(case.W, case.H, threads=4, depth=run.depth, samples=1)
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
                set_sampled_hit_lighting(o, run, k, on, none=[])
                f["rays_" + name] = o.ray_trace()
                f[name] = HOST.oracle_words(o)
            out.append(f)
        return out
    finally:
        o.close()


def hit_run_primary_passes(run, k, scene, m):
    """The model's primary passes that run behind the hit sum in a whole frame of the run (the device's frames have them: where they add
    nothing the "off" frame's word IS the word in front of S)."""
    out = []
    if run.sun is not None:
        out.append(R.sun_pass(scene, run.case.constants(k), m, SR.normalise(run.sun(k)[0]), run.sun(k)[1], angle_degrees=run.angle))
    if run.lights is not None:
        out.append((R.list_pass if run.as_list else R.pick_pass if run.mode == 1 else R.lights_pass)(scene, run.case.constants(k), m, light_dicts(run.lights(k))))
    return out


def measure_sampled_hits(run, frames=None):
    """The hit stage's check (test_shading_paths_host.check_hit_stage, the delta of the scene's paths at the run's depth) on every frame of a
    hit run -> its entry of the floor table."""
    import test_shading_paths_host as PATHS
    case = run.case
    frames = run_sampled_hit_restatement(run) if frames is None else frames
    scene = R.Scene(case.meshes, case.cube)
    models = PATHS.model_frames(SC.PathRun(case, run.depth, 1), [f["off"]["vis"] for f in frames])
    bounds = PATHS.hit_bounds(run)
    used, counts, share = {}, {}, 0.0
    for k, f, m in zip(run.positions, frames, models):
        label = "%s frame %d" % (run.name, SC.FRAMES[k])
        sun = (SR.normalise(run.sun(k)[0]), run.sun(k)[1]) if run.sun is not None else None
        p = R.hits_pass(scene, case.constants(k), m, sun, light_dicts(run.lights(k)) if run.lights is not None else (), sun_angle=run.angle, mode=run.mode)
        sh = float(((p["flags"] != 0) & m["covered"]).sum()) / max(int(m["covered"].sum()), 1)
        share = max(share, sh)
        assert sh <= FLAG_CAP, "%s: %.2f %% of the covered pixels flagged (%s): change the case, not the cap" % (
            label, 100 * sh, {n: int(((p["flags"] & b) != 0).sum()) for b, n in R.FLAG_NAMES.items() if ((p["flags"] & b) != 0).any()})
        flagged = int((p["flags"] != 0).sum())
        per_hit = 1 if run.mode == 1 or run.lights is None else LR.MAX_LIGHTS
        if "rays_on" in f:
            assert abs((f["rays_on"] - f["rays_off"]) - p["rays"]) <= 2 * per_hit * flagged * run.depth, "%s: %d shadow rays from hits, the model %d" % (
                label, f["rays_on"] - f["rays_off"], p["rays"])
        for img, (a, b) in PATHS.check_hit_stage(label, f["off"], f["on"], p, bounds, f.get("only")).items():
            t = used.setdefault(img, [0, 0]); t[0] += a; t[1] += b
        for (lev, name), v in p["counts"].items():
            key = "terms_level_%d" % lev if name in R.LOBES else name
            counts[key] = counts.get(key, 0) + v
    for name, least in REACH_HITS.items():
        assert counts.get(name, 0) >= least, "%s reaches %s %d times, asked %d (%s)" % (run.name, name, counts.get(name, 0), least, counts)
    if run.mode == 1:
        assert counts.get("two_candidates", 0) >= 100 and (not run.as_list or counts.get("chosen_from_8", 0) >= 20), "%s: %s" % (run.name, counts)
    return {"family": run.family, "flagged_share_max": share, "reach": counts}, used


def floor_bounds(cases):
    """Per family: the pick's from its measured terms (not below one ulp: the add's own rounding); the disk's and the radii's from the floor of
    the same scenes' ray-traced path, as the directional passes' (DELTA_FROM)."""
    base = HOST.recorded()["bounds"]
    out = {fam: {key: {"max": base[src][key]["max"]} for key in ("refl", "diff")} for fam, src in DELTA_FROM.items()}
    for fam in ("pick", "list", "records"):
        mine = [c for c in cases.values() if c["family"] == fam and "refl" in c]
        if mine:
            out[fam] = {key: {"max": max(1.0, max(c[key]["max"] for c in mine))} for key in ("refl", "diff")}
    return out


def write_floor():
    doc = {"about": "the sampled lights against the float64 model: per run what it reaches (conditions, tests/test_shading_sampled_host.py REACH), the largest share "
                    "of flagged pixels of a pass, and -- the pick -- fp32 ulps (of the pixel's largest channel) by which the restatement's terms S0, S1 differ from "
                    "the model's interval on unflagged pixels; bounds: the code rule's delta per family, x margin",
           "margin": MARGIN, "flag_cap": FLAG_CAP, "pick_eps": R.PICK_EPS, "delta_from": DELTA_FROM, "cases": {}, "bounds": {}}
    old = json.load(open(FLOOR_PATH)) if os.path.exists(FLOOR_PATH) else {}
    # (the pick's stage check needs its own bounds: measured first with the lights' delta in their place)
    doc["bounds"] = floor_bounds({})
    with open(FLOOR_PATH, "w") as f:
        json.dump(dict(doc, bounds=dict(doc["bounds"], pick=HOST.recorded()["bounds"]["lights"], list=HOST.recorded()["bounds"]["lights"], records=HOST.recorded()["bounds"]["lights"])), f)
    try:
        doc["cases"] = {run.name: measure(run)[0] for run in SC.sampled_cases()}
        doc["cases"].update({run.name: measure_records(run)[0] for run in SC.record_cases()})
        doc["cases"].update({run.name: measure_sampled_hits(run)[0] for run in SC.sampled_hit_cases()})
    finally:
        doc["bounds"] = floor_bounds(doc["cases"]) if doc["cases"] else doc["bounds"]
        if "gpu_measured" in old:
            doc["gpu_measured"] = old["gpu_measured"]
        with open(FLOOR_PATH, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    return doc


def recorded():
    return json.load(open(FLOOR_PATH))


@pytest.mark.parametrize("name", SC.SAMPLED_NAMES)
def test_sampled_pass_against_the_restatement_and_the_recorded_floor(name):
    run = SC.sampled_by_name(name)
    rec = recorded()
    assert (rec["margin"], rec["flag_cap"], rec["pick_eps"]) == (MARGIN, FLAG_CAP, R.PICK_EPS)
    got, used = measure(run)
    print("%s: %s %s" % (name, json.dumps(got), json.dumps(used)))
    _check_against_recorded(name, got, used, rec["cases"][name])


def _check_against_recorded(name, got, used, want):
    assert got["family"] == want["family"] and got["reach"] == want["reach"] and got["terms"] == want["terms"] and got["rays"] == want["rays"]
    assert got["flagged_share_max"] <= FLAG_CAP and all(b > 0 for _, b in used.values())
    for key in ("refl", "diff"):
        if key in want:
            assert got[key]["n"] == want[key]["n"], "%s %s: number of compared pixels" % (name, key)
            for q in HOST.QUANTS:      # a measurement: last bits of libm and numpy move it; what is asked is that it has not grown
                assert got[key][q] <= FLOOR_DRIFT * want[key][q] + 0.5, "%s %s %s: the floor grew: %.3f, recorded %.3f" % (name, key, q, got[key][q], want[key][q])


@pytest.mark.parametrize("name", [r.name for r in SC.record_cases()])
def test_record_sequence_one_frame_at_a_time_against_the_restatement(name):
    """Seven acting frames with a moving camera and instance, a reset by rtggx_set_lights in the middle and one frame whose image read the test
    has overwritten with random bytes (the restatement's images can be written; the product has rtggx_read_light_visibility and no way to
    write, so the device's sequence runs without that frame's overwrite)."""
    run = next(r for r in SC.record_cases() if r.name == name)
    got, used = measure_records(run)
    print("%s: %s %s" % (name, json.dumps(got), json.dumps(used)))
    _check_against_recorded(name, got, used, recorded()["cases"][name])


@pytest.mark.parametrize("name", [r.name for r in SC.sampled_hit_cases()])
def test_sampled_targets_at_the_hits_against_the_restatement(name):
    """The court at D = 2: the sun's slots 1 + 2 d + i at 5 degrees; the lights' 32 + 16 d + 8 img + i with radii and mode 1's hit rule
    (w_i = Y(T_d term_i), the draw from 104 + 2 d + img, the term s_i f); the list's 8192 + 1024 (2 d + img) + i from light 8 on."""
    run = next(r for r in SC.sampled_hit_cases() if r.name == name)
    got, used = measure_sampled_hits(run)
    print("%s: %s %s" % (name, json.dumps(got), json.dumps(used)))
    want = recorded()["cases"][name]
    assert got["reach"] == want["reach"] and got["flagged_share_max"] <= FLAG_CAP and all(b > 0 for _, b in used.values())


def test_recorded_bounds_follow_from_the_recorded_cases_and_the_cases_reach_what_they_were_built_for():
    rec = recorded()
    assert sorted(rec["cases"]) == sorted(SC.SAMPLED_NAMES + tuple(r.name for r in SC.record_cases() + SC.sampled_hit_cases())) and rec["bounds"] == floor_bounds(rec["cases"]) and rec["delta_from"] == DELTA_FROM
    assert MARGIN <= 4.0
    for run in SC.record_cases():
        check_record_reach(run, rec["cases"][run.name]["reach"])
        assert rec["cases"][run.name]["flagged_share_max"] <= FLAG_CAP and len(run.indices) >= 6 and run.scramble
        assert any(run.lights(j) is not None for j in range(2, len(run.indices) - 1)), "no reset in the middle"
    for run in SC.sampled_cases():
        check_reach(run, rec["cases"][run.name]["reach"])
        assert rec["cases"][run.name]["flagged_share_max"] <= FLAG_CAP
    # the cases as the issue lists them: every sun at every angle; a dark light inside a list; radii small, near the height, on a spot; metallic on both sides of 1
    suns = {(k, a) for r in SC.sampled_cases() if r.kind == "sun" for k in r.positions for _, a in r.passes(k)}
    assert suns == {(k, a) for k in range(3) for a in (0.27, 5.0, 10.0)}
    low = SR.normalise(SC.sampled_by_name("sun_disk_75x53").case.sun(1)[0])
    assert 0.005 < float(low[1]) < 0.015      # NoL 0.01 on the slab: every disk of 5 and 10 degrees dips below its horizon
    assert {len(r.lights(0)) for r in SC.sampled_cases() if r.kind == "list"} == {12, 65, 200}
    soft = SC.sampled_by_name("radii_75x53")
    for k in range(3):
        ls = soft.lights(k)
        assert any(max(l["intensity"]) == 0 and 0 < i < len(ls) - 1 for i, l in enumerate(ls)) or k == 0
    assert any(l.get("radius", 0) > 0 and l.get("cos_outer", -1) > -1 for l in soft.lights(0))
    B = next(l for l in soft.lights(1) if tuple(l["position"]) == (-1.0, -0.75, -0.5))
    assert 0.25 < B["radius"] < 1.5 * 0.25      # the light is 0.25 above the slab (y = -1): its sphere dips into it
    pick = SC.sampled_by_name("pick_75x53")
    assert {len(pick.lights(k)) for k in range(3)} >= {2, 8}
    metals = {float(mt[2]) for mt in pick.case.materials(0)}
    assert any(x < 1.0 for x in metals) and any(x >= 1.0 for x in metals)
    assert (pick.case.W, pick.case.H) == (75, 53)


# ---- a: known answers ------------------------------------------------------------------------------------------------------------------
def _frame_of(L):
    """Exact T and B of the header's rule, unrounded."""
    a = np.zeros(3); a[int(np.argmin(np.abs(L)))] = 1.0
    T = np.cross(a, L); T /= np.linalg.norm(T)
    return T, np.cross(L, T)


@pytest.mark.parametrize("degrees", [0.27, 5.0, 10.0])
def test_the_disk_map_is_uniform_in_solid_angle_and_stays_inside_the_cap(degrees):
    L = np.array([0.36, 0.48, 0.8])
    T, B = _frame_of(L)
    k = 1.0 - np.cos(np.radians(degrees))
    g = np.linspace(0.05, 0.95, 10)
    u, v = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    h_of = lambda a, b: R.sun_disk_direction(L, k, T, B, a, 2 * np.pi * b)
    # the cap's solid angle is 2 pi k: the image of the unit square's uniform density is 1 / (2 pi k) everywhere
    step = 1e-4
    coarse, fine = HOST._density_by_jacobian(h_of, u, v, step), HOST._density_by_jacobian(h_of, u, v, step / 2)
    want = 1.0 / (2.0 * np.pi * k)
    tol = 2.0 * np.abs(coarse - fine) + 1e-6 * want      # (the difference's own error; 1e-6: its cancellation at a step of 5e-5 in double)
    assert (np.abs(fine - want) <= tol).all(), "the disk map's density is off by up to %.3g (relative)" % np.max(np.abs(fine - want) / want)
    # with exact T and B every Ls is a unit vector; the map is right-handed about L (phi runs from T towards B = L x T)
    # (every sixteenth u, and the sixteen nearest the rim, with every entry of the table)
    every_u, every_phi = np.meshgrid(np.concatenate([np.arange(0, 65536, 16), np.arange(65520, 65536)]) / 65536.0, 2 * np.pi * np.arange(256) / 256.0, indexing="ij")
    Ls = R.sun_disk_direction(L, k, T, B, every_u.reshape(-1), every_phi.reshape(-1))
    assert np.abs(np.sqrt((Ls * Ls).sum(axis=1)) - 1.0).max() <= 1e-6
    q = R.sun_disk_direction(L, k, T, B, np.array([0.5, 0.5]), np.array([0.0, 0.5 * np.pi]))
    assert np.dot(np.cross(q[0] - L, q[1] - L), L) > 0.0
    # with the host's rounded k, T, B (what the device is given) every Ls lies inside the cap
    kk, Tr, Br = R.sun_disk_host(L.astype(np.float32), degrees)
    Lf = L.astype(np.float32).astype(np.float64)
    Ls = R.sun_disk_direction(Lf, kk, Tr, Br, every_u.reshape(-1), every_phi.reshape(-1))
    assert (Ls @ Lf >= np.cos(np.radians(degrees)) - 1e-7).all()
    assert (Ls @ Lf).min() <= np.cos(np.radians(degrees)) + 2.0 * k / 65536.0 + 1e-7, "the rim is never reached"


def test_the_sphere_map_has_the_uniform_spheres_moments():
    """Over the full enumeration u = j / 65536, s = 0 .. 255: z = 1 - 2 u has the mean 2^-16 exactly (the u are the left ends of their
    cells) and the second moment (N^2 + 2) / (3 N^2), N = 65536; the 256 azimuths are equally spaced, so every moment that is odd in
    x or y vanishes and x^2, y^2 share 1 - E z^2 equally.  What remains is the sums' rounding in double: 1e-12."""
    N = 65536
    u, phi = np.meshgrid(np.arange(N) / float(N), 2 * np.pi * np.arange(256) / 256.0, indexing="ij")
    o = R.sphere_point(u.reshape(-1), phi.reshape(-1))
    np.testing.assert_allclose((o * o).sum(axis=1), 1.0, atol=1e-12)
    np.testing.assert_allclose(o.mean(axis=0), [0.0, 0.0, 2.0 ** -16], atol=1e-12)
    zz = (N * N + 2.0) / (3.0 * N * N)
    np.testing.assert_allclose(o.T @ o / len(o), np.diag([0.5 * (1 - zz), 0.5 * (1 - zz), zz]), atol=1e-12)
    assert abs(zz - 1.0 / 3.0) < 2e-10 and abs(0.5 * (1 - zz) - 1.0 / 3.0) < 2e-10      # I / 3 to the table's discretisation


@pytest.mark.parametrize("offset", [-0.8, -0.4, 0.0, 0.4, 0.8])
def test_a_penumbras_lit_share_is_the_caps_share_beyond_the_edges_plane(offset):
    """A straight occluder edge along z at height h over a slab, the occluder on the side x < 0, a zenith sun of 5 degrees; a point of the
    slab at x = offset x (the penumbra's half width h tan 5deg).  The ray along Ls passes the occluder's height at x + h Ls.x / Ls.y and is
    lit where that is > 0.  In the cap's own coordinates (theta from L, phi' from B = +x) that is sin(theta) cos(phi') / cos(theta) > -x / h:
    for a fixed theta the lit share of the azimuth is arccos(c) / pi with c = clamp(-x / (h tan(theta))), and cos(theta) = 1 - u k is uniform
    in u (uniform in solid angle), so the lit share of the cap's solid angle is the integral of that over u in [0, 1] -- taken here by the
    midpoint rule at 2^20 points.  The enumeration of all (u, s) replaces the azimuth's share by the count of the 256 equally spaced table
    entries inside one arc, which differs from 256 x the arc's share by less than 1: the bound is 1 / 256."""
    degrees, h = 5.0, 0.7
    L = np.array([0.0, 1.0, 0.0])
    kk, T, B = R.sun_disk_host(L.astype(np.float32), degrees)
    np.testing.assert_array_equal(T, [0.0, 0.0, 1.0]); np.testing.assert_array_equal(B, [1.0, 0.0, 0.0])      # a = x (ties to the lowest index): T = x cross y, B = y cross T
    x = offset * h * np.tan(np.radians(degrees))
    u, phi = np.meshgrid(np.arange(65536) / 65536.0, 2 * np.pi * np.arange(256) / 256.0, indexing="ij")
    Ls = R.sun_disk_direction(L, kk, T, B, u.reshape(-1), phi.reshape(-1))
    lit = float((x + h * Ls[:, 0] / Ls[:, 1] > 0.0).mean())
    um = (np.arange(2 ** 20) + 0.5) / 2 ** 20
    ct = 1.0 - um * (1.0 - np.cos(np.radians(degrees)))
    tan_t = np.sqrt(1.0 - ct * ct) / ct
    want = float((np.arccos(np.clip(-x / (h * tan_t), -1.0, 1.0)) / np.pi).mean())
    assert abs(lit - want) <= 1.0 / 256.0, "offset %g: lit share %.5f, the cap's share %.5f" % (offset, lit, want)
    if offset == 0.0:
        assert abs(want - 0.5) < 1e-9
    else:
        assert 0.02 < want < 0.98 and abs(want - 0.5) > 0.1      # (a map with another radius would show here)


def _pick_measure(weights):
    """Per light the number of the 2^24 draws x = j / 2^24 that choose it, by the model's pick_choice."""
    w = np.asarray(weights, np.float64)
    counts = np.zeros(len(w), np.int64)
    for a in range(0, 1 << 24, 1 << 20):
        x = np.arange(a, a + (1 << 20)) / 16777216.0
        chosen, _, _ = R.pick_choice(x, np.repeat(w[:, None], len(x), axis=1))
        counts += np.bincount(chosen, minlength=len(w))
    return counts


@pytest.mark.parametrize("weights, bytes_", [
    ((0.3, 1.7), None), ((2.5e-3, 0.0, 4.0, 1e-4), None), ((1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0), None),
    ((0.3, 1.7), (0, 255)), ((1.0, 1.0, 1.0, 1.0), (0, 15, 16, 255)), ((0.5, 0.0, 0.25, 8.0, 1e-3), (255, 7, 0, 16, 15))])
def test_the_pick_is_unbiased_from_the_integer_measure_of_its_draws(weights, bytes_):
    """sum_i P(i) f_i term_i = sum_i term_i in luminance (Y(term_i) = w_i, so each product is W): P(i) is the share of the 2^24 draws that
    choose light i, off from w_i / W by at most 2^-24 at each of its two boundaries -- n 2^-24 relative over n candidates, with room for the
    sums' rounding.  With the remembered visibility the pick weights are u_i = w_i max(v_i, 16): the identity holds for any bytes."""
    w = np.asarray(weights, np.float64)
    u = w if bytes_ is None else R.visibility_weights(w, np.asarray(bytes_))
    if bytes_ is not None:
        np.testing.assert_array_equal(u, w * np.maximum(np.asarray(bytes_), 16))
        assert (u[w > 0] > 0).all()      # the floor: every candidate keeps a probability
    counts = _pick_measure(u)
    assert counts.sum() == 1 << 24 and (counts[u == 0] == 0).all() and (counts[u > 0] > 0).all()
    U = u.sum()
    cand = u > 0
    estimate = (counts[cand] / 16777216.0 * (U / u[cand]) * w[cand]).sum()
    n = int(cand.sum())
    assert abs(estimate - w.sum()) <= (n + 1) * 2.0 ** -24 * (U / u[cand]).max() * w.sum()
    assert abs((counts[cand] / 16777216.0 * (U / u[cand]) * u[cand]).sum() - U) <= (n + 1) * 2.0 ** -24 * U


def test_a_single_candidate_has_f_exactly_one_and_the_last_candidate_is_the_fallback():
    x = np.array([0.0, 0.5, 1.0 - 2.0 ** -24])
    chosen, W, c = R.pick_choice(x, np.repeat(np.array([0.0, 0.37, 0.0])[:, None], 3, axis=1))
    assert chosen.tolist() == [1, 1, 1] and (W / 0.37 == 1.0).all()
    # t = x W can round up to W = c_last in fp32; the rule then takes the last CANDIDATE, not the last light
    chosen, _, _ = R.pick_choice(np.array([1.0]), np.array([[1.0], [2.0], [0.0]]))
    assert chosen.tolist() == [1]
    assert R.pick_choice(np.array([0.3]), np.zeros((3, 1)))[0].tolist() == [-1]


def test_the_update_rule_reaches_0_and_255_exactly_and_stays():
    v = np.arange(256)
    assert R.visibility_update(255, True) == 255 and R.visibility_update(0, False) == 0
    up, down = v.copy(), v.copy()
    for _ in range(64):
        nu, nd = R.visibility_update(up, True), R.visibility_update(down, False)
        assert (nu >= up).all() and (nd <= down).all() and (nu[up < 255] > up[up < 255]).all() and (nd[down > 0] < down[down > 0]).all()
        up, down = nu, nd
    assert (up == 255).all() and (down == 0).all()


def test_the_slot_sets_are_pairwise_disjoint():
    sun = {R.sun_slot()} | {R.sun_slot(d, i) for d in range(4) for i in range(2)}
    primary = {R.light_slot(i) for i in range(1024)}
    hits = {R.light_hit_slot(d, img, i) for d in range(4) for img in range(2) for i in range(1024)}
    draws = {R.SLOT_PICK} | {R.pick_hit_slot(d, img) for d in range(4) for img in range(2)}
    assert sun == set(range(9)) and {s for s in primary if s < 4096} == set(range(16, 24)) and {s for s in hits if s < 8192} == set(range(32, 96))
    assert draws == {96} | set(range(104, 112)) and len(primary) == 1024 and len(hits) == 8 * 1024
    sets = (sun, primary, hits, draws)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not (sets[a] & sets[b])
    # the words themselves: the model's integer hash against the restatement's, over slots of every set
    for pixel, index, slot in ((0, 0, 0), (3974, 255, 96), (1234, 1, 23), (77, 2047, 8192 + 7 * 1024 + 1023)):
        assert int(R.slot_words(np.array([pixel]), index, slot)[0]) == LP.draw_word_lib(pixel, index, slot) == LP.draw_word(pixel, index, slot)
