"""The HIP shading path at recursion depth 2 to 4 and 2 to 8 samples per pixel against the CPU restatement AND the float64 model
(tests/shading_ref.py follow_paths), per pixel, on the runs of shading_cases.path_cases(): closed rooms whose paths run to the last level
under both samplers, a black metallic room (the preset rule), open sky with misses at level 1, the coincident sheets and the apex met by
deeper rays, skewed and mirrored instances (the hit's own inverse transpose), 8, 4 and 2 samples (frame index 255 at N = 8: FrameIndex N + k up
to 2047), samples x depth.

Every other test of rtggx_set_max_recursion_depth and rtggx_set_samples_per_pixel compares the kernels with tests/recursion_ref.cpp and
tests/spp_ref.cpp alone, which restate them line by line.  Here, for every frame of every run, through a bare context (gpu_support.Scene)
with restatement.Oracle(depth, samples) beside it:
  * the G-buffer words, RayTracingOut0 / 1 and the ray count equal the restatement's bit for bit;
  * on the pixels the model does not flag, every stored code obeys the code rule against the model's value (test_shading_ref_host
    check_words; delta = the run's recorded floor maximum x 2, tests/golden/shading_paths_floor.json, measured on the restatement's fp32
    values by tests/test_shading_paths_host.py);
  * what a frame does not write stays, bit for bit.
One context per run; sheets_vertex at depth 2 once more as a strip that begins at row 35; materials_3 and materials_1 at depth 2 with 2
samples once more at the traversal's resident shape, in a child process (tests/shading_paths_resident_child.py).

The sun and the lights at the hits (shading_cases.hit_cases(): sun_75x53, lights_75x53 and the walled court at depth 1 and 2, each kind and
both at once): see run_hits.

The values that use the one-code allowance are recorded per run in the floor file's `gpu_measured` entry by write_gpu_measured (by hand,
on a GPU, after a deliberate change of the kernels)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_support as G
import restatement as RS
import shading_ref as R
import shading_cases as SC
import test_shading_paths_host as PATHS
import test_shading_ref_host as HOST
from test_gpu_shading_synthetic import ORACLE_IDS, STRIP_FIRST_ROW, WORDS

pytestmark = pytest.mark.gpu

RESIDENT_RUNS = ("materials_3_64x48_d2n2", "materials_1_64x48_d2n2")


def run_path(run, strip_from=None):
    """Every frame of a run through one context beside one restatement -> {word name: (values that used the allowance, values compared)}."""
    from oracle import oracle as O
    case = run.case
    bounds = PATHS.bounds_of(run)
    rows = slice(strip_from, case.H) if strip_from is not None else slice(None)
    strip = (strip_from, case.H) if strip_from is not None else None
    s = G.Scene(*case.meshes, *[w.astype(np.float32) for w in case.worlds(0)], size=(case.W, case.H),
                oracle=lambda w, h: RS.Oracle(w, h, depth=run.depth, samples=run.samples, entry="spp"))
    frames = []
    try:
        s.set_cube(case.cube, case.vndf)
        s.ctx.set_max_recursion_depth(run.depth); s.ctx.set_samples_per_pixel(run.samples)
        for k in run.positions:
            label = "%s frame %d%s" % (run.name, SC.FRAMES[k], "" if strip_from is None else ", rows from %d" % strip_from)
            w, rays, want_rays = s.shaded_frame(case.constants(k), case.materials(k), strip=strip)
            ow = {n: s.o.buffer(getattr(O, ORACLE_IDS[n])) for n in WORDS}
            for n in WORDS:
                np.testing.assert_array_equal(w[n][rows], ow[n][rows], err_msg="%s: %s not bit-exact" % (label, n))
            if strip_from is None:
                assert rays == want_rays, "%s: %d rays, the restatement %d" % (label, rays, want_rays)
            frames.append((label, w, ow["vis"]))      # (outside a strip the device's rows are not the frame's: the model runs on the whole frame's visibility)
    finally:
        s.close()
    used = {}
    cut = lambda d: {n: (v[rows] if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[:2] == (case.H, case.W) else v) for n, v in d.items()}
    prev = None
    for (label, w, _), m in zip(frames, PATHS.model_frames(run, [f[2] for f in frames])):
        assert HOST.flagged_share(m) <= HOST.FLAG_CAP, label
        for name, (a, b) in HOST.check_words(label, cut(w), cut(m), None if prev is None else cut(prev), bounds).items():
            t = used.setdefault(name, [0, 0]); t[0] += a; t[1] += b
        prev = w
    return used


def run_hits(run):
    """Every frame of a hit run through one context beside tests/light_hit_ref.py's restatement, the switches of its kind off, then on, in the
    same context: both frames bit for bit the restatement's (every word, the ray count), and the hit sum's stage against the model through
    the device's words -- where the primary passes of rtggx_set_sun / rtggx_set_lights add nothing (the model's sun_pass / lights_pass: no
    term, no flag), the word of the "off" frame IS the word in front of S and the stage is one rounding; elsewhere those passes re-round
    the word behind S and the stage is judged on the restatement's words in front of them (tests/test_shading_paths_host.py), which the
    device's equal.  -> {image: (values that used the allowance, values compared)}."""
    from oracle import oracle as O
    import light_hit_ref as LH
    case = run.case
    s = G.Scene(*case.meshes, *[w.astype(np.float32) for w in case.worlds(0)], size=(case.W, case.H), oracle=lambda w, h: LH.Oracle(w, h, depth=run.depth, samples=1))
    frames = []
    try:
        s.set_cube(case.cube, case.vndf)
        s.ctx.set_max_recursion_depth(run.depth)
        for k in run.positions:
            f = {}
            for name, on in (("off", 0), ("on", 1)):
                label = "%s frame %d, switches %s" % (run.name, SC.FRAMES[k], name)
                PATHS.set_hit_lighting(s.o, run, k, on)
                s.ctx.set_sun(*(run.sun(k) if run.sun is not None else (None, None)))
                s.ctx.set_lights(run.lights(k) if run.lights is not None else None)
                s.ctx.set_sun_reflections(1 if on and run.sun is not None else 0); s.ctx.set_light_reflections(1 if on and run.lights is not None else 0)
                w, rays, want_rays = s.shaded_frame(case.constants(k), case.materials(k))
                for n in WORDS:
                    np.testing.assert_array_equal(w[n], s.o.buffer(getattr(O, ORACLE_IDS[n])), err_msg="%s: %s not bit-exact" % (label, n))
                assert rays == want_rays, "%s: %d rays, the restatement %d" % (label, rays, want_rays)
                f[name] = w
            frames.append(f)
    finally:
        s.close()
    scene = R.Scene(case.meshes, case.cube)
    for k, f, (m, _) in zip(run.positions, frames, PATHS.hit_models(run, [f["off"]["vis"] for f in frames])):
        only = np.stack([m["flags"] == 0, m["flags"] == 0])
        if run.sun is not None:
            q = R.sun_pass(scene, case.constants(k), m, *PATHS.hit_sun(run, k))
            only &= np.stack([~q["term"], ~q["diffuse"]]) & (q["flags"] == 0)
        if run.lights is not None:
            q = R.lights_pass(scene, case.constants(k), m, PATHS.hit_lights(run, k))
            only &= np.stack([~q["term"], ~q["diffuse"]]) & (q["flags"] == 0)
        f["only"] = only
    return PATHS.measure_hits(run, frames)[1]


@pytest.mark.parametrize("name", SC.HIT_NAMES)
def test_hit_run_bit_for_bit_with_the_restatement_and_its_stage_with_the_model(built, name):
    used = run_hits(SC.hit_by_name(name))
    print("%s: %s" % (name, json.dumps(used)))
    want = PATHS.recorded()["gpu_measured"]["hit_runs"][name]
    for img, (a, b) in used.items():
        assert b == want[img][1] and a <= 1.25 * want[img][0] + 5, "%s %s: the one-code allowance used %d times of %d, recorded %s" % (name, img, a, b, want[img])
    if name.startswith("court"):
        assert all(b >= 300 for _, b in used.values()), "%s: too few values where the primary passes add nothing: %s" % (name, used)


@pytest.mark.parametrize("name", SC.PATH_NAMES)
def test_run_bit_for_bit_with_the_restatement_and_per_pixel_with_the_model(built, name):
    used = run_path(SC.path_by_name(name))
    print("%s: %s" % (name, json.dumps(used)))
    assert all(b > 0 for _, b in used.values())
    # the allowance is used as often as when the device was measured (its words are the restatement's, so this moves only with the model's last bits)
    want = PATHS.recorded()["gpu_measured"]["runs"][name]
    for word, (a, b) in used.items():
        assert b == want[word][1] and a <= 1.25 * want[word][0] + 5, "%s %s: the one-code allowance used %d times of %d, recorded %s" % (name, word, a, b, want[word])


def test_depth_2_as_a_strip_that_begins_at_row_35(built):
    """The kernels' first row is not row 0, at every level: open sky, the sheets and the cone inside the strip or across its edge."""
    used = run_path(SC.path_by_name("sheets_vertex_96x64_d2n1"), strip_from=STRIP_FIRST_ROW)
    assert all(b > 0 for _, b in used.values())


def test_samples_and_depth_at_the_resident_shape(built):
    """Two samples of two levels once more with the traversal's resident workgroups (12 waves per CU, tree tops in LDS): these frames trace
    fewer than RT_TINY_RAYS rays per launch; RTGGX_TRACE_WAVES, read once per process, forces the shape: hence a fresh child process."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "shading_paths_resident_child.py")],
                       env=dict(os.environ, RTGGX_TRACE_WAVES="12"), capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "resident paths ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def write_gpu_measured(commit, path=PATHS.FLOOR_PATH):
    """The device's use of the one-code allowance per run and word, into the `gpu_measured` entry of tests/golden/shading_paths_floor.json:

        python -c "import sys; sys.path[:0] = ['tests', '.']; import test_gpu_shading_paths as t; t.write_gpu_measured('<the commit it ran on>')"
    """
    doc = PATHS.recorded()
    runs = {run.name: {w: [int(a), int(b)] for w, (a, b) in run_path(run).items()} for run in SC.path_cases()}
    hits = {run.name: {w: [int(a), int(b)] for w, (a, b) in run_hits(run).items()} for run in SC.hit_cases()}
    doc["gpu_measured"] = {"measured_on": commit, "device": "MI355X (gfx950)", "margin": HOST.MARGIN, "runs": runs, "hit_runs": hits}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc["gpu_measured"]
