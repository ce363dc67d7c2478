"""The HIP shading path against the CPU oracle AND the float64 model (tests/shading_ref.py), per pixel, on the synthetic scenes of
tests/shading_cases.py: non-uniform and mirrored instance transforms, normals around the up-vector switch, at grazing angles and turned
away, 13 roughness codes, metallic on both sides of 0.5 and at 1, colours with zero channels and above 1, cubes of 1, 3 and 5 mips, a
closed room and open sky, a shared vertex on a pixel centre, coincident sheets, both samplers, a ProjBias, moving camera and instance,
a sun and up to eight local lights over a slab with an occluder.

Every other frame test compares the kernels with the oracle alone, which restates them line by line, on the bunny or the dragon under
uniform transforms.  Here, for every frame (indices 0, 1, 255) of every case, through a bare context (gpu_support.Scene):
  * the G-buffer words, RayTracingOut0 / 1 and the ray count equal the oracle's bit for bit;
  * on the pixels the model does not flag, every stored code obeys the code rule against the model's value (test_shading_ref_host
    check_words: at most one code off, and only within delta of a rounding boundary; delta = the family's recorded floor maximum x 2 --
    tests/golden/shading_synthetic_floor.json, measured on the oracle's fp32 values by tests/test_shading_ref_host.py);
  * what a frame does not write (RayTracingOut1 under metallic 1, the rough-metal word where nothing is drawn) stays, bit for bit.
One context per case (a context has one size and one pair of meshes); one case once more as a strip that begins at row 35; the
materials family once more at the traversal's resident shape, in a child process (test_materials_at_the_resident_shape).

The share of values that use the one-code allowance is written per family into the floor file's `gpu_measured` entry by write_gpu_measured
(by hand, on a GPU, after a deliberate change of the kernels)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_support as G
import shading_cases as SC
import test_shading_ref_host as HOST

pytestmark = pytest.mark.gpu

WORDS = ("vis", "depth", "normal", "rm", "velocity", "refl", "diff")
ORACLE_IDS = {"vis": "BUF_VISIBILITY", "depth": "BUF_DEPTH", "normal": "BUF_NORMAL", "rm": "BUF_ROUGH_METAL", "velocity": "BUF_VELOCITY", "refl": "BUF_RT_REFL", "diff": "BUF_RT_DIFF"}
STRIP_FIRST_ROW = 35


def run_case(case, strip_from=None):
    """Every frame of a case through one context beside one oracle -> {word name: (values that used the allowance, values compared)}."""
    from oracle import oracle as O
    bounds = HOST.recorded()["bounds"][case.family]
    rows = slice(strip_from, case.H) if strip_from is not None else slice(None)
    direct = case.sun is not None or case.lights is not None
    oracle = None
    if direct:      # the restatement that carries the sun and the lights (tests/lights_ref.py)
        import lights_ref as LR
        oracle = lambda w, h: LR.Oracle(w, h)
    s = G.Scene(*case.meshes, *[w.astype(np.float32) for w in case.worlds(0)], size=(case.W, case.H), oracle=oracle)
    frames, stages = [], []
    strip = (strip_from, case.H) if strip_from is not None else None

    def one(label, k):
        w, rays, want_rays = s.shaded_frame(case.constants(k), case.materials(k), strip=strip)
        ow = {n: s.o.buffer(getattr(O, ORACLE_IDS[n])) for n in WORDS}
        for n in WORDS:
            np.testing.assert_array_equal(w[n][rows], ow[n][rows], err_msg="%s: %s not bit-exact" % (label, n))
        if strip_from is None:
            assert rays == want_rays, "%s: %d rays, the oracle %d" % (label, rays, want_rays)
        return w, ow["vis"]
    try:
        s.set_cube(case.cube, case.vndf)
        for k in range(len(SC.FRAMES)):
            label = "%s frame %d%s" % (case.name, SC.FRAMES[k], "" if strip_from is None else ", rows from %d" % strip_from)
            if direct:
                s.ctx.set_sun(None, None); s.o.set_sun(None, None); s.ctx.set_lights(None); s.o.set_lights([])
            w, vis = one(label, k)
            frames.append((label, w, vis))      # (outside a strip the device's rows are not the frame's: the model runs on the whole frame's visibility)
            st = [("base", dict(w, vis=vis), None)]
            if case.sun is not None:      # the same frame once more with the sun, then with the lights as well: each pass's own arithmetic
                s.ctx.set_sun(*case.sun(k)); s.o.set_sun(*case.sun(k))
                st.append(("sun", one(label + " with the sun", k)[0], None))
            if case.lights is not None:
                s.ctx.set_lights(case.lights(k)); s.o.set_lights(case.lights(k))
                st.append(("lights", one(label + " with the lights", k)[0], None))
            stages.append(st)
            frames[-1] += (st[-1][1],)      # what the context holds when the next frame begins: a carry-over is of the LAST frame run, sun and lights included
    finally:
        s.close()
    used = {}
    cut = lambda d: {n: (v[rows] if isinstance(v, np.ndarray) and v.ndim >= 2 else v) for n, v in d.items()}
    prev = None
    for (label, w, _, last), m in zip(frames, HOST.model_frames(case, [f[2] for f in frames])):
        assert HOST.flagged_share(m) <= HOST.FLAG_CAP, label
        for name, (a, b) in HOST.check_words(label, cut(w), cut(m), None if prev is None else cut(prev), bounds).items():
            t = used.setdefault(name, [0, 0]); t[0] += a; t[1] += b
        prev = last
    if direct and strip_from is None:
        for name, (a, b) in HOST.check_direct(case, stages)[0].items():
            used[name] = [a, b]
    return used


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_bit_for_bit_with_the_oracle_and_per_pixel_with_the_model(built, name):
    used = run_case(SC.by_name(name))
    print("%s: %s" % (name, json.dumps(used)))
    assert all(b > 0 for _, b in used.values())
    # the allowance is used as often as when the device was measured (its words are the oracle's, so this moves only with the model's last bits)
    want = HOST.recorded()["gpu_measured"]["cases"][name]
    for word, (a, b) in used.items():
        assert b == want[word][1] and a <= 1.25 * want[word][0] + 5, "%s %s: the one-code allowance used %d times of %d, recorded %s" % (name, word, a, b, want[word])


def test_a_strip_that_begins_at_row_35(built):
    """The kernels' first row is not row 0: the hits family's case (96 x 64, open sky; the sheets and the cone inside the strip or across its edge)."""
    used = run_case(SC.by_name("sheets_vertex_96x64"), strip_from=STRIP_FIRST_ROW)
    assert all(b > 0 for _, b in used.values())


def test_materials_at_the_resident_shape(built):
    """Family 3 once more with the traversal's resident workgroups (12 waves per CU, tree tops in LDS): these frames trace fewer than
    RT_TINY_RAYS rays and would launch single-wave workgroups; RTGGX_TRACE_WAVES, read once per process, forces the shape: hence a child."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "shading_resident_child.py")],
                       env=dict(os.environ, RTGGX_TRACE_WAVES="12"), capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "resident shading ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def write_gpu_measured(commit, path=HOST.FLOOR_PATH):
    """The device's share of values that use the one-code allowance, per family and word, into the `gpu_measured` entry of
    tests/golden/shading_synthetic_floor.json:

        python -c "import sys; sys.path[:0] = ['tests', '.']; import test_gpu_shading_synthetic as t; t.write_gpu_measured('<the commit it ran on>')"
    """
    doc = HOST.recorded()
    cases = {case.name: {w: [int(a), int(b)] for w, (a, b) in run_case(case).items()} for case in SC.all_cases()}
    fam = {}
    for family in SC.FAMILIES:
        used = {}
        for case in SC.all_cases():
            if case.family == family:
                for name, (a, b) in cases[case.name].items():
                    t = used.setdefault(name, [0, 0]); t[0] += a; t[1] += b
        fam[family] = {name: {"allowance_used": a, "compared": b, "share": a / max(b, 1)} for name, (a, b) in used.items()}
    doc["gpu_measured"] = {"measured_on": commit, "device": "MI355X (gfx950)", "margin": HOST.MARGIN, "families": fam, "cases": cases}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return doc["gpu_measured"]
