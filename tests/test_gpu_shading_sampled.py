"""The sampled lights on the GPU against their restatements AND the float64 model (tests/shading_ref.py), per pixel, on
shading_cases.sampled_cases(): the sun's disk (rtggx_set_sun_angle), the lights' radii, the light pick (rtggx_set_light_sampling(ctx, 1))
and the culled list (rtggx_set_light_list).  Every other test of these features compares the kernels with a restatement written beside
them; here, for every frame (indices 0, 1, 255) of every run, through a bare context (gpu_support.Scene):
  * the frame without the feature, then the same frame with it -- the switch toggled within one context -- give the words in front of the
    pass and behind it; both, and the ray counts, equal the restatement's bit for bit;
  * on the pixels the model does not flag, the device's own words obey the stage check of tests/test_shading_sampled_host.py (the code rule
    on base + term, the words untouched where the model adds nothing), and the pass's shadow rays are the model's;
  * the list: rtggx_read_light_list_counts lies per block within the model's [certain, certain + uncertain] (shading_ref.cull_counts); with
    rtggx_debug_light_list_cull(ctx, 0) every block that has a covered pixel reads the number of casting lights and the images are the same.
  * the visibility records (rtggx_set_light_pick_visibility): a sequence of seven acting frames, judged one frame at a time -- the image read
    from the device in front of the frame, the image written and the sequence behind it, exact; the words against a twin context that runs
    the same frames without lights.
  * the sampled targets at the hits (the court at depth 2: the sun at 5 degrees, lights with radii in mode 1, a list of 12), the hit
    switches off and then on, where the primary passes add nothing.
One pick run once more as a strip from row 35 (pixel is the full-frame index; the records are refused on a strip), and once more at the
traversal's resident shape, in a child process.

The share of values that use the one-code allowance goes into tests/golden/shading_sampled_floor.json's `gpu_measured` entry, by hand on a
GPU after a deliberate change of the kernels (write_gpu_measured)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_support as G
import shading_cases as SC
import test_shading_ref_host as HOST
import test_shading_sampled_host as T

pytestmark = pytest.mark.gpu

WORDS = ("vis", "normal", "rm", "velocity", "refl", "diff")
ORACLE_IDS = {"vis": "BUF_VISIBILITY", "normal": "BUF_NORMAL", "rm": "BUF_ROUGH_METAL", "velocity": "BUF_VELOCITY", "refl": "BUF_RT_REFL", "diff": "BUF_RT_DIFF"}
STRIP_FIRST_ROW = 35


def run_device(run, strip_from=None, cull=True):
    """Every frame of a run through one context beside the restatement (tests/light_list_ref.py), the feature off and then on -> the stages
    in run_restatement's shape, of the DEVICE's words; everything is asserted bit for bit with the restatement on the way."""
    import light_list_ref as LL
    from oracle import oracle as O
    case = run.case
    rows = slice(strip_from, case.H) if strip_from is not None else slice(None)
    strip = (strip_from, case.H) if strip_from is not None else None
    s = G.Scene(*case.meshes, *[w.astype(np.float32) for w in case.worlds(0)], size=(case.W, case.H), oracle=lambda w, h: LL.Oracle(w, h))

    def one(label, k):
        w, rays, want_rays = s.shaded_frame(case.constants(k), case.materials(k), strip=strip)
        ow = {n: s.o.buffer(getattr(O, ORACLE_IDS[n])) for n in WORDS}
        for n in WORDS:
            np.testing.assert_array_equal(w[n][rows], ow[n][rows], err_msg="%s: %s not bit-exact" % (label, n))
        if strip_from is None:
            assert rays == want_rays, "%s: %d rays, the restatement %d" % (label, rays, want_rays)
        return dict(w, vis=ow["vis"]), rays      # (outside a strip the device's rows are not the frame's: the model runs on the whole frame's visibility)

    try:
        s.set_cube(case.cube, case.vndf)
        if not cull:
            s.ctx.debug_light_list_cull(0)
        out = []
        for k in run.positions:
            for x in (s.ctx, s.o):
                x.set_sun(None, None); x.set_lights(None if x is s.ctx else []); x.set_light_list(None if x is s.ctx else []); x.set_sun_angle(0.0); x.set_light_sampling(0)
            base, base_rays = one("%s frame %d" % (run.name, SC.FRAMES[k]), k)
            stages = [("base", base, base_rays, {})]
            for what, angle in run.passes(k):
                label = "%s frame %d, %s" % (run.name, SC.FRAMES[k], what)
                for x in (s.ctx, s.o):
                    if run.kind == "sun":
                        x.set_sun(*case.sun(k)); x.set_sun_angle(angle)
                    elif run.kind == "list":
                        x.set_light_list(run.lights(k))
                    else:
                        x.set_lights(run.lights(k)); x.set_light_sampling(1 if run.kind == "pick" else 0)
                w, rays = one(label, k)
                o = s.o
                told = {"sun": lambda: {"classes": o.classes.copy()}, "lights": lambda: {"classes": o.light_classes.copy()},
                        "pick": lambda: {"info": o.pick_info.copy(), "wf": o.pick_wf.copy(), "terms": o.pick_terms.copy()},
                        "list": lambda: {"info": o.list_info.copy(), "wf": o.list_wf.copy(), "terms": o.list_terms.copy()}}[run.kind]()
                if run.kind == "list" and strip_from is None:
                    told["kept"] = s.ctx.read_light_list_counts()      # the DEVICE's counts, for the model's bounds
                    if cull:
                        np.testing.assert_array_equal(told["kept"], o.list_kept, err_msg="%s: kept lights per block" % label)
                stages.append((what, w, rays - base_rays if strip_from is None else None, told))
            out.append(stages)
        return out
    finally:
        s.close()


def run_record_device(run):
    """Every frame of a record run through one context beside the restatement (tests/light_vis_ref.py) and a twin context that runs the same
    frames without lights -- a successful rtggx_set_lights is a reset, so the switch cannot be toggled: the twin's words stand in front of
    the pass -- -> frames in run_record_restatement's shape, of the DEVICE's words and records; bit for bit with the restatement on the
    way.  The image (s - 1) & 1 is read from the device in front of the frame, the image s & 1 and the sequence behind it.  The product
    has no way to write the records: no frame's image is overwritten here."""
    import light_list_ref as LL
    import light_vis_ref as LV
    from oracle import oracle as O
    case = run.case
    make = lambda orc: G.Scene(*case.meshes, *[w.astype(np.float32) for w in case.worlds(0)], size=(case.W, case.H), oracle=lambda w, h: orc(w, h))
    s = make(LV.Oracle)
    try:
        twin = make(LL.Oracle)
    except Exception:
        s.close()
        raise
    try:
        for x in (s, twin):
            x.set_cube(case.cube, case.vndf)
        for x in (s.ctx, s.o):
            x.set_light_sampling(1); x.set_light_pick_visibility(1)
        out = []
        for j, index in enumerate(run.indices):
            label = "%s frame %d (index %d)" % (run.name, j, index)
            if run.lights(j) is not None:
                s.ctx.set_lights(run.lights(j)); s.o.set_lights(run.lights(j))
            held = np.zeros((2, case.H, case.W), T.R.RECORD)
            if out:      # (before the first acting frame nothing is allocated and the read is refused: the images are zero)
                held[0], held[1] = s.ctx.read_light_visibility(0)[0], s.ctx.read_light_visibility(1)[0]
            np.testing.assert_array_equal(held.view(np.uint8), s.o.images.view(np.uint8), err_msg="%s: the record images in front of the frame" % label)
            fc = case.constants(j, index)
            before, base_rays, want_base = twin.shaded_frame(fc, case.materials(j))
            w, rays, want_rays = s.shaded_frame(fc, case.materials(j))
            assert (base_rays, rays) == (want_base, want_rays), "%s: %d and %d rays, the restatements %d and %d" % (label, base_rays, rays, want_base, want_rays)
            for n in WORDS:
                np.testing.assert_array_equal(w[n], s.o.buffer(getattr(O, ORACLE_IDS[n])), err_msg="%s: %s not bit-exact" % (label, n))
                np.testing.assert_array_equal(before[n], twin.o.buffer(getattr(O, ORACLE_IDS[n])), err_msg="%s: the twin's %s not bit-exact" % (label, n))
            seq = s.ctx.read_light_visibility(0)[1]
            new = s.ctx.read_light_visibility(seq & 1)[0]
            assert seq == s.o.seq, "%s: sequence %d, the restatement's %d" % (label, seq, s.o.seq)
            np.testing.assert_array_equal(new.view(np.uint8), s.o.images[seq & 1].view(np.uint8), err_msg="%s: the record image written" % label)
            np.testing.assert_array_equal(s.ctx.read_light_visibility((seq - 1) & 1)[0].view(np.uint8), held[(seq - 1) & 1].view(np.uint8), err_msg="%s: the image read was written" % label)
            out.append({"before": before, "after": w, "rays": rays - base_rays, "read": held[(seq - 1) & 1], "old": held[seq & 1], "new": new, "seq": seq,
                        "told": {"info": s.o.pick_info.copy(), "terms": s.o.pick_terms.copy(), "wf": s.o.pick_wf.copy()}})
        return out
    finally:
        s.close(); twin.close()


def device_record_run(run):
    return SC.RecordRun(run.name, run.case, run.indices, run.lights, scramble=())


@pytest.mark.parametrize("name", [r.name for r in SC.record_cases()])
def test_record_sequence_bit_for_bit_and_one_frame_at_a_time_with_the_model(built, name):
    run = device_record_run(next(r for r in SC.record_cases() if r.name == name))
    got, used = T.measure_records(run, run_record_device(run))
    print("%s: %s %s" % (name, json.dumps(got["reach"]), json.dumps(allowance(used))))
    assert all(b > 0 for _, b in used.values())
    want = T.recorded()["gpu_measured"]["cases"][name]
    for word, (a, b) in used.items():
        assert b == want[word][1] and a <= 1.25 * want[word][0] + 5, "%s %s: the one-code allowance used %d times of %d, recorded %s" % (name, word, a, b, want[word])


def run_sampled_hits_device(run):
    """Every frame of a hit run through one context beside the restatement, the hit switches off, then on, in the same context: both frames
    bit for bit the restatement's (every word, the ray count) -> frames for T.measure_sampled_hits, of the DEVICE's words, judged where
    the primary passes behind the hit sum add nothing (tests/test_gpu_shading_paths.py run_hits has the reason)."""
    import light_list_ref as LL
    import test_shading_paths_host as PATHS
    from oracle import oracle as O
    case = run.case
    s = G.Scene(*case.meshes, *[w.astype(np.float32) for w in case.worlds(0)], size=(case.W, case.H), oracle=lambda w, h: LL.Oracle(w, h, depth=run.depth, samples=1))
    frames = []
    try:
        s.set_cube(case.cube, case.vndf)
        s.ctx.set_max_recursion_depth(run.depth)
        for k in run.positions:
            f = {}
            for name, on in (("off", 0), ("on", 1)):
                label = "%s frame %d, switches %s" % (run.name, SC.FRAMES[k], name)
                T.set_sampled_hit_lighting(s.o, run, k, on, none=[])
                T.set_sampled_hit_lighting(s.ctx, run, k, on, none=None)
                w, rays, want_rays = s.shaded_frame(case.constants(k), case.materials(k))
                for n in WORDS:
                    np.testing.assert_array_equal(w[n], s.o.buffer(getattr(O, ORACLE_IDS[n])), err_msg="%s: %s not bit-exact" % (label, n))
                assert rays == want_rays, "%s: %d rays, the restatement %d" % (label, rays, want_rays)
                f[name] = w
            frames.append(f)
    finally:
        s.close()
    scene = T.R.Scene(case.meshes, case.cube)
    models = PATHS.model_frames(SC.PathRun(case, run.depth, 1), [f["off"]["vis"] for f in frames])
    for k, f, m in zip(run.positions, frames, models):
        only = np.stack([m["flags"] == 0, m["flags"] == 0])
        for q in T.hit_run_primary_passes(run, k, scene, m):
            only &= np.stack([~q["term"], ~q["diffuse"]]) & (q["flags"] == 0)
        f["only"] = only
    return frames


@pytest.mark.parametrize("name", [r.name for r in SC.sampled_hit_cases()])
def test_sampled_hits_bit_for_bit_with_the_restatement_and_their_stage_with_the_model(built, name):
    run = next(r for r in SC.sampled_hit_cases() if r.name == name)
    got, used = T.measure_sampled_hits(run, run_sampled_hits_device(run))
    print("%s: %s" % (name, json.dumps(allowance(used))))
    assert all(b >= 300 for _, b in used.values()), "%s: too few values where the primary passes add nothing: %s" % (name, used)
    want = T.recorded()["gpu_measured"]["cases"][name]
    for word, (a, b) in used.items():
        assert b == want[word][1] and a <= 1.25 * want[word][0] + 5, "%s %s: the one-code allowance used %d times of %d, recorded %s" % (name, word, a, b, want[word])


def allowance(used):
    return {name: [int(a), int(b)] for name, (a, b) in used.items()}


@pytest.mark.parametrize("name", SC.SAMPLED_NAMES)
def test_run_bit_for_bit_with_the_restatement_and_per_pixel_with_the_model(built, name):
    run = SC.sampled_by_name(name)
    got, used = T.measure(run, run_device(run))
    print("%s: %s %s" % (name, json.dumps(got["reach"]), json.dumps(allowance(used))))
    rec = T.recorded()
    assert got["reach"] == rec["cases"][name]["reach"] and got["rays"] == rec["cases"][name]["rays"] and got["terms"] == rec["cases"][name]["terms"]
    assert all(b > 0 for _, b in used.values())
    # the allowance is used as often as when the device was measured (its words are the restatement's, so this moves only with the model's last bits)
    want = rec["gpu_measured"]["cases"][name]
    for word, (a, b) in used.items():
        assert b == want[word][1] and a <= 1.25 * want[word][0] + 5, "%s %s: the one-code allowance used %d times of %d, recorded %s" % (name, word, a, b, want[word])


def test_the_list_with_the_cull_off(built):
    """Every casting light kept in every block that has a covered pixel, and the same images: both runs' words equal the restatement's, which
    has no cull, bit for bit (run_device), and here each other's."""
    run = SC.sampled_by_name("list_65_75x53")
    on, off = run_device(run), run_device(run, cull=False)
    casting = sum(1 for l in run.lights(0) if max(l["intensity"]) > 0)
    scene_models = HOST.model_frames(run.case, [st[0][1]["vis"] for st in off])
    for k, (a, b, m) in enumerate(zip(on, off, scene_models)):
        for key in ("refl", "diff"):
            np.testing.assert_array_equal(a[1][1][key], b[1][1][key], err_msg="frame %d: %s with the cull off" % (k, key))
        assert a[1][2] == b[1][2]
        cull = T.R.cull_counts(m, T.light_dicts(run.lights(k)))
        T.check_cull("list_65 frame %d, cull off" % k, cull, b[1][3]["kept"], casting, cull_on=False)
        assert (a[1][3]["kept"] < casting).any()
    T.measure(run, off, cull_on=False)


def test_a_pick_as_a_strip_that_begins_at_row_35(built):
    """The kernels' first row is not row 0 and `pixel` is still the full-frame index: the rows of the strip equal the restatement's whole
    frame bit for bit (run_device) and obey the stage check against the model of the whole frame.  The records are refused on a strip."""
    from raytracedggx_amd import capi
    run = SC.sampled_by_name("pick_radii_75x53")
    frames = run_device(run, strip_from=STRIP_FIRST_ROW)
    case = run.case
    scene = T.R.Scene(case.meshes, case.cube)
    models = HOST.model_frames(case, [st[0][1]["vis"] for st in frames])
    rows = slice(STRIP_FIRST_ROW, case.H)
    cut = lambda d: {n: (v[rows] if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[0] == case.H else v) for n, v in d.items()}
    compared = 0
    for k, stages, m in zip(run.positions, frames, models):
        p = T.model_pass(run, k, scene, m)
        used = HOST.check_direct_stage("%s frame %d, rows from %d" % (run.name, SC.FRAMES[k], STRIP_FIRST_ROW), cut(stages[0][1]), cut(stages[1][1]), cut(p), T.bounds_of(run))
        compared += sum(b for _, b in used.values())
    assert compared > 1000
    ctx = capi.Context(case.W, case.H)
    try:
        ctx.set_strip(STRIP_FIRST_ROW, case.H)
        with pytest.raises(capi.RtggxError, match="rtggx_set_light_pick_visibility"):
            ctx.set_light_pick_visibility(1)
    finally:
        ctx.close()


def test_a_pick_at_the_resident_shape(built):
    """One pick run once more with the traversal's resident workgroups (12 waves per CU, tree tops in LDS): these frames trace fewer than
    RT_TINY_RAYS rays and would launch single-wave workgroups; RTGGX_TRACE_WAVES, read once per process, forces the shape: hence a fresh child."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "shading_sampled_resident_child.py")],
                       env=dict(os.environ, RTGGX_TRACE_WAVES="12"), capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "resident sampled shading ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def write_gpu_measured(commit, path=T.FLOOR_PATH):
    """The device's share of values that use the one-code allowance, per run and image, into the `gpu_measured` entry of
    tests/golden/shading_sampled_floor.json:

        python -c "import sys; sys.path[:0] = ['tests', '.']; import test_gpu_shading_sampled as t; t.write_gpu_measured('<the commit it ran on>')"
    """
    doc = T.recorded()
    cases = {run.name: allowance(T.measure(run, run_device(run))[1]) for run in SC.sampled_cases()}
    cases.update({run.name: allowance(T.measure_records(device_record_run(run), run_record_device(device_record_run(run)))[1]) for run in SC.record_cases()})
    cases.update({run.name: allowance(T.measure_sampled_hits(run, run_sampled_hits_device(run))[1]) for run in SC.sampled_hit_cases()})
    fam = {}
    for run in SC.sampled_cases() + SC.record_cases() + SC.sampled_hit_cases():
        for name, (a, b) in cases[run.name].items():
            t = fam.setdefault(run.family, {}).setdefault(name, {"allowance_used": 0, "compared": 0})
            t["allowance_used"] += a; t["compared"] += b
    for f in fam.values():
        for t in f.values():
            t["share"] = t["allowance_used"] / max(t["compared"], 1)
    doc["gpu_measured"] = {"measured_on": commit, "device": "MI355X (gfx950)", "margin": T.MARGIN, "families": fam, "cases": cases}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc["gpu_measured"]
