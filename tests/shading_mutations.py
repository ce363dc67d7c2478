"""Mutation proof of the shading model's assertions, as a host proxy (like profiles/r09_env_mutations.txt): each mutation below is applied to
a scratch copy of the CPU oracle -- the twin line of the kernel's -- which is compiled and put in the kernel's place in the code rule of
tests/test_shading_ref_host.py (check_words against the float64 model on unflagged pixels, the GPU test's own assertion).  Bit equality with
itself would pass every one of them; a mutation no case catches means a missing case.  Run by hand, it writes the report:

    python tests/shading_mutations.py depth1 profiles/r20_shading_mutations.txt

The last two are lines of the sun's and the lights' restatements (tests/sun_ref.cpp, tests/lights_ref.cpp) and are judged by the stage check
of those passes (check_direct).  PATH_MUTATIONS (the second report, profiles/r22_shading_path_mutations.txt) are lines of the path
follower and the sample loop.  SAMPLED_MUTATIONS (profiles/r24_sampled_light_mutations.txt) are lines of the sampled lights' restatements.  """
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

import light_hit_ref as LH
import lights_ref as LR
import restatement as RS
import shading_cases as SC
import test_shading_paths_host as PATHS
import test_shading_ref_host as HOST
from oracle import oracle as O

# (name, [(text of oracle/orc_raytrace.h, its replacement), ...]) or (name, edits, file under tests/); every text must occur
MUTATIONS = (
    ("WorldIT -> World", [("cb_load3x3(h.inst ? c.fc.g.WorldIT1 : c.fc.g.WorldITs0)", "cb_load4x3(c.fc.g.Worlds[h.inst])"),
                          ("cb_load3x3(s.inst ? fc.g.WorldIT1 : fc.g.WorldITs0)", "cb_load4x3(fc.g.Worlds[s.inst])")]),
    ("the SH's -norm.x -> norm.x", [("const float x = -norm.x,", "const float x = norm.x,")]),
    ("fSchlick's 50 -> 5", [("const float s = saturate(50.0f * spec.y) * fc;", "const float s = saturate(5.0f * spec.y) * fc;")]),
    ("visSmith's a2 -> a", [("const float a = roughness * roughness, a2 = a * a;", "const float a = roughness * roughness, a2 = a;")]),
    ("the up-vector threshold 0.999 -> 0.9", [("std::fabs(n.y) < 0.999f", "std::fabs(n.y) < 0.9f")]),
    ("the checkerboard's 0.25 -> 0.5", [("rough * 0.25f", "rough * 0.5f")]),
    ("1.15 -> 1.0 in the mip rule", [("3.0f - 1.15f * log2Contract(rgh)", "3.0f - 1.0f * log2Contract(rgh)")]),
    ("lerp3's factor without + a", [("(1.0f - a) * (std::sqrt(1.0f - a) + a)", "(1.0f - a) * (std::sqrt(1.0f - a))")]),
    ("0.04 -> 0.4", [("lerp(0.04f,", "lerp(0.4f,")]),
    ("the diffuse (1 - 0.04) dropped", [("col * (s.color * (1.0f - 0.04f))", "col * (s.color)")]),
    ("reflect3(-V, Hh) -> reflect3(V, Hh)", [("reflect(-s.V, Hh)", "reflect(s.V, Hh)")]),
    ("4 VoH / NoH -> 4 VoH", [("const float k = 4.0f * VoH / NoH;", "const float k = 4.0f * VoH;")]),
    ("the light's q q -> q", [("float win = saturate(1.0f - q * q);", "float win = saturate(1.0f - q);")], "lights_ref.cpp"),
    ("the sun's max(r, 1/32) dropped", [("const float r = std::fmax(rghMtl.x, 1.0f / 32.0f);", "const float r = rghMtl.x;")], "sun_ref.cpp"),
)

# Lines of the path follower and the sample loop (tests/recursion_ref.cpp, tests/spp_ref.cpp: the twins of raytrace.hip's levels and samples),
# judged by the runs of shading_cases.path_cases() against the model's paths (tests/test_shading_paths_host.py): the code rule on unflagged
# pixels and the model's ray count.  Written by the second argument:
#
#     python tests/shading_mutations.py paths profiles/r22_shading_path_mutations.txt
PATH_MUTATIONS = (
    ("T * w -> w alone", [("T = f3(T.x * w.x, T.y * w.y, T.z * w.z);", "T = w;")], "recursion_ref.cpp"),
    ("w = color -> color (1 - 0.04) at depth >= 1", [("w = color;  ", "w = color * (1.0f - 0.04f);  ")], "recursion_ref.cpp"),
    ("the diffuse group's (1 - m) dropped", [("if (diffuseGroup) color = color * (1.0f - rm.y);", ";")], "recursion_ref.cpp"),
    ("the last level's (1 - m) dropped", [("diffuseGroup ? color * (1.0f - rm.y) : color", "color")], "recursion_ref.cpp"),
    ("the preset test with || instead of &&", [("preset.x <= 0.0f && preset.y <= 0.0f && preset.z <= 0.0f", "preset.x <= 0.0f || preset.y <= 0.0f || preset.z <= 0.0f")], "recursion_ref.cpp"),
    ("the preset of the previous surface", [("    preset = color * rm.y;\n", "")], "recursion_ref.cpp"),
    ("the skip id left at the primary's", [("o = P; dir = L; skipInst = h.inst; skipPrim = h.prim;", "o = P; dir = L;")], "recursion_ref.cpp"),
    ("d + 1 == D -> d == D", [("if (d + 1 == D) {", "if (d == D) {")], "recursion_ref.cpp"),
    ("V = -dir -> the first ray's V", [("    const float3 V = -dir;\n", "    static thread_local float3 V0; if (d == 0) V0 = -dir; const float3 V = V0;\n")], "recursion_ref.cpp"),
    ("FrameIndex N + k -> FrameIndex + k", [("fc.g.FrameIndex * N + k", "fc.g.FrameIndex + k")], "spp_ref.cpp"),
    ("1 / N -> 1 / (N - 1)", [("const float scale = 1.0f / (float)N;", "const float scale = 1.0f / (float)(N > 1 ? N - 1 : 1);")], "spp_ref.cpp"),
    ("the sum started at sample 1", [("for (uint32_t k = 0; k < N; ++k) {", "for (uint32_t k = (N > 1 ? 1 : 0); k < N; ++k) {")], "spp_ref.cpp"),
)


# Lines of the lights' and the sun's terms at the hits (tests/light_hit_ref.cpp), judged by the stage check of the hit runs (measure_hits)
HIT_MUTATIONS = (
    ("the hit term's color' without (1 - m)", [("    if (diffuseGroup) color = color * (1.0f - rm.y);\n    const float g = (NoL / kPI) * att;", "    const float g = (NoL / kPI) * att;")]),
    ("the hit term with x 0.96", [("const float g = (NoL / kPI) * att;", "const float g = ((NoL / kPI) * att) * (1.0f - 0.04f);")]),
    ("s_d without T_d (a light's)", [("  S = f3(S.x + T.x * term.x, S.y + T.y * term.y, S.z + T.z * term.z);\n  return LC_LIT;", "  S = f3(S.x + term.x, S.y + term.y, S.z + term.z);\n  return LC_LIT;")]),
    ("s_d without T_d (the sun's)", [("            S = f3(S.x + T.x * term.x, S.y + T.y * term.y, S.z + T.z * term.z);\n            any = true;", "            S = f3(S.x + term.x, S.y + term.y, S.z + term.z);\n            any = true;")]),
    ("a light's hit interval to 1e4 instead of tmax", [("trace_closest(c, P, Ls, 1e-5f, tmax, hInst, hPrim)", "trace_closest(c, P, Ls, 1e-5f, 10000.0f, hInst, hPrim)")]),
)


# Lines of the sampled lights' restatements, judged by the stage checks of tests/test_shading_sampled_host.py (measure, measure_records,
# measure_sampled_hits) on the runs named: (name, file under tests/, [(text, replacement), ...], kind of run that judges it).  Written by
#
#     python tests/shading_mutations.py sampled profiles/r24_sampled_light_mutations.txt
_DISK = "f3((K.T.x * ct + K.B.x * st) + L.x * cosTheta, (K.T.y * ct + K.B.y * st) + L.y * cosTheta, (K.T.z * ct + K.B.z * st) + L.z * cosTheta)"
_NO_RAY = "if (rc) { if (rec.info) rec.info[pix * 4 + 2] = rc; return 0; }      // no ray: v as carried"
SAMPLED_MUTATIONS = (
    ("T and B exchanged", "sun_soft_ref.cpp", [(_DISK, _DISK.replace("K.T.", "K.X.").replace("K.B.", "K.T.").replace("K.X.", "K.B."))], "sun"),
    ("sqrt(e (2 - e)) -> sqrt(e)", "sun_soft_ref.cpp", [("std::sqrt(e * (2.0f - e))", "std::sqrt(e)")], "sun"),
    ("u from w >> 16", "sun_soft_ref.cpp", [("const float u = (float)(w & 0xffffu) / 65536.0f;", "const float u = (float)(w >> 16) / 65536.0f;")], "sun"),
    ("s = w >> 24 -> w & 0xff", "sun_soft_ref.cpp", [("const uint32_t s = w >> 24;", "const uint32_t s = w & 0xffu;")], "sun"),
    ("the sun's second test dot(N, Ls) > 0 dropped", "sun_soft_ref.cpp", [("if (!(dot(N, Ls) > 0.0f)) { if (classes) classes[pix] = 4; return 0; }", "")], "sun"),
    ("z = 1 - 2u -> 1 - u", "lights_ref.cpp", [("const float z = 1.0f - 2.0f * u;", "const float z = 1.0f - u;")], "lights"),
    ("Ds = D + rho o -> D - rho o", "lights_ref.cpp", [("Ds = f3(D.x + l.rho * o.x, D.y + l.rho * o.y, D.z + l.rho * o.z);", "Ds = f3(D.x - l.rho * o.x, D.y - l.rho * o.y, D.z - l.rho * o.z);")], "lights"),
    ("slot 16 + i -> 16", "lights_ref.cpp", [("rng(h + (16u + i) * 0x9E3779B9u)", "rng(h + (16u) * 0x9E3779B9u)")], "lights"),
    ("tmax = sqrt(ds2) -> sqrt(d2)", "lights_ref.cpp", [("const float tmax = std::sqrt(ds2);", "const float tmax = std::sqrt(d2);")], "lights"),
    ("Y = 0.25/0.5/0.25 -> thirds", "light_pick_ref.cpp", [("return (0.25f * c.x + 0.5f * c.y) + 0.25f * c.z;", "return ((1.0f / 3.0f) * c.x + (1.0f / 3.0f) * c.y) + (1.0f / 3.0f) * c.z;")], "pick"),
    ("w_i without Y(diff_i)", "light_pick_ref.cpp", [("      wi = wi + pick_luminance(diff[i]);\n    }\n    if (!(wi > 0.0f)) continue;      // (a NaN is not a candidate)",
                                                      "    }\n    if (!(wi > 0.0f)) continue;")], "pick"),
    ("f = W / w_i -> 1", "light_pick_ref.cpp", [("const float f = Wsum / w[ch];\n  if (rec.info)", "const float f = 1.0f;\n  if (rec.info)")], "pick"),
    ("f from the first candidate's weight", "light_pick_ref.cpp", [("const float f = Wsum / w[ch];\n  if (rec.info)",
                                                                     "float w0 = 0.0f; for (int q = 7; q >= 0; --q) if (cand[q]) w0 = w[q];\n  const float f = Wsum / w0;\n  if (rec.info)")], "pick"),
    ("draw slot 96 -> 16", "light_pick_ref.cpp", [("pick_word((uint32_t)pix, frameIndex, 96u)) * Wsum;", "pick_word((uint32_t)pix, frameIndex, 16u)) * Wsum;")], "pick"),
    ("x = v >> 8 -> v & 0xffffff", "light_pick_ref.cpp", [("(float)(v >> 8) / 16777216.0f", "(float)(v & 0xffffffu) / 16777216.0f")], "pick"),
    ("\"else the last candidate\" -> the first candidate", "light_pick_ref.cpp", [("if (fallback) chosen = last;", "if (fallback) chosen = first;")], "pick"),
    ("the visibility floor 16 -> 0", "light_vis_ref.cpp", [("(float)(vi > kVisFloor ? vi : kVisFloor)", "(float)vi")], "records"),
    ("max(v, floor) -> v + floor", "light_vis_ref.cpp", [("(float)(vi > kVisFloor ? vi : kVisFloor)", "(float)(vi + kVisFloor)")], "records"),
    (">> 2 -> >> 1 in the update", "light_vis_ref.cpp", [("v - ((v + 3u) >> 2) : v + ((255u - v + 3u) >> 2)", "v - ((v + 3u) >> 1) : v + ((255u - v + 3u) >> 1)")], "records"),
    ("the update applied where no ray was traced", "light_vis_ref.cpp",
     [(_NO_RAY, "if (rc) { const uint32_t sh = 8u * ((uint32_t)ch & 3u); mine[ch >> 2] = (mine[ch >> 2] & ~(0xFFu << sh)) | (vis_update(before, true) << sh); "
                "if (rec.info) rec.info[pix * 4 + 2] = rc; return 0; }")], "records"),
    ("history read from image s & 1", "light_vis_ref.cpp", [("R = prev + 4u * ((size_t)(uint32_t)qy * W_ + (uint32_t)qx);", "R = next + 4u * ((size_t)(uint32_t)qy * W_ + (uint32_t)qx);")], "records"),
    ("- vx W -> + vx W", "light_vis_ref.cpp", [("std::floor(((float)px + 0.5f) - vx * (float)W_)", "std::floor(((float)px + 0.5f) + vx * (float)W_)")], "records"),
    ("the normal threshold 0.9 -> 0", "light_vis_ref.cpp", [(">= 0.9f * 1046529.0f", ">= 0.0f * 1046529.0f")], "records"),
    ("the inst + 1 test dropped", "light_vis_ref.cpp", [("else if ((R[3] & 0xFFu) != inst + 1u) cls = VC_INSTANCE;", "")], "records"),
    ("no reset on set_lights", "light_vis_ref.cpp", [("if (!(s - 1u > s0)) cls = VC_SEQUENCE;", "if (!(s - 1u > 0u)) cls = VC_SEQUENCE;")], "records"),
    ("list slot 4096 + i -> 16 + (i & 7)", "light_list_ref.cpp", [("return i < 8u ? 16u + i : 4096u + i;", "return 16u + (i & 7u);")], "list"),
    ("hit draw slot 104 + 2d + img -> 96", "light_pick_ref.cpp", [("pick_word(pixel, frameIndex, 104u + 2u * d + image)) * Wsum;", "pick_word(pixel, frameIndex, 96u)) * Wsum;")], "hits"),
    ("w_i = Y(T_d term_i) -> Y(term_i)", "light_pick_ref.cpp", [("const float wi = pick_luminance(s[i]);", "const float wi = pick_luminance(term);")], "hits"),
)
# A mutant no stage check can catch, with the reason: in fp32 the fallback branch is dead.
EQUIVALENT = {
    "\"else the last candidate\" -> the first candidate":
        "equivalent: the branch is never taken.  x <= 1 - 2^-24, so x W <= W - W 2^-24, and with W in [2^k, 2^(k+1)) the spacing below W is at most 2^(k-23) <= 2 W 2^-24: "
        "x W lies at or below the midpoint of pred(W) and W, strictly below it unless W = 2^k, where W - 2^(k-24) is itself a number; round-to-nearest gives t <= pred(W) < W, "
        "and the last running sum c is W bit for bit (the same additions in the same order), so a candidate with t < c always exists.  The model's own fallback is held by "
        "test_a_single_candidate_has_f_exactly_one_and_the_last_candidate_is_the_fallback.",
}


def first_sampled_failure(edits, work, file, kind):
    """(run, message) of the first run of the mutation's kind whose stage check fails on the mutated restatement, or None."""
    import light_list_ref as LL
    import light_vis_ref as LV
    import test_shading_sampled_host as S
    own = LL._lib, LV._lib
    LL.lib(); LV.lib()
    try:
        if kind == "records":
            LV._lib = mutated_library(edits, work, file, "light_vis_ref.cpp", LV.lib())
        else:
            LL._lib = mutated_library(edits, work, file, "light_list_ref.cpp", LL.lib())
        if kind == "records":
            runs = [(r, S.measure_records) for r in SC.record_cases()]
        elif kind == "hits":
            runs = [(r, S.measure_sampled_hits) for r in SC.sampled_hit_cases()]
        else:
            runs = [(r, S.measure) for r in SC.sampled_cases() if r.kind == kind]
        for run, judge in runs:
            try:
                judge(run)
            except AssertionError as e:
                return run.name, re.sub(r"\s+", " ", str(e).split(", first")[0])[:260]
    finally:
        LL._lib, LV._lib = own
    return None


def sampled_main(path):
    lines = ["Mutations of the sampled lights' CPU restatements (the twin lines of lighting.hip: the sun's disk, the lights' radii, the pick, the visibility",
             "records, the list's slots, mode 1 at the hits) against the float64 model's stage checks on unflagged pixels -- the code rule on base + term, the",
             "ray's class and the chosen light per pixel, the records exactly, the shadow-ray count (tests/shading_mutations.py; the unmutated restatements pass",
             "every run: tests/test_shading_sampled_host.py).", ""]
    with tempfile.TemporaryDirectory() as work:
        for kind in ("sun", "records"):
            clean = first_sampled_failure([], work, None, kind)
            assert clean is None, "the unmutated copy fails: %s" % (clean,)
        lines.append("%-52s passes" % "(no mutation)")
        missed = []
        for name, file, edits, kind in SAMPLED_MUTATIONS:
            got = first_sampled_failure(edits, work, file, kind)
            if got is None and name in EQUIVALENT:
                lines.append("%-52s not caught; %s" % (name, EQUIVALENT[name]))
            else:
                lines.append("%-52s %s" % (name, "NOT CAUGHT" if got is None else "caught, first by %s" % got[1]))
                if got is None:
                    missed.append(name)
    lines += ["", "%d of %d caught, %d equivalent" % (len(SAMPLED_MUTATIONS) - len(missed) - len(EQUIVALENT), len(SAMPLED_MUTATIONS), len(EQUIVALENT))]
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if missed else 0


def mutated_library(edits, work, file=None, source="lights_ref.cpp", signatures=None):
    """The whole oracle and every restatement (tests/lights_ref.cpp includes them all; source: another top file) from a scratch copy with the
    edits applied."""
    for d in ("oracle", "tests"):
        if os.path.exists(os.path.join(work, d)):
            shutil.rmtree(os.path.join(work, d))
    shutil.copytree(O._HERE, os.path.join(work, "oracle"), ignore=shutil.ignore_patterns("_build", "_ref", "__pycache__"))
    os.makedirs(os.path.join(work, "tests"))
    for f in os.listdir(LR._HERE):
        if f.endswith(".cpp"):
            shutil.copy(os.path.join(LR._HERE, f), os.path.join(work, "tests", f))
    path = os.path.join(work, "tests", file) if file else os.path.join(work, "oracle", "orc_raytrace.h")
    text = open(path).read()
    for old, new in edits:
        assert old in text, old
        text = text.replace(old, new)
    open(path, "w").write(text)
    out = os.path.join(work, "libmutant_%d.so" % len(os.listdir(work)))
    subprocess.check_call([os.environ.get("CXX", "g++")] + RS._FLAGS + ["-shared", "-pthread", "-o", out, os.path.join(work, "tests", source)])
    L = C.CDLL(out)
    for name, fn in list(vars(signatures or LR.lib()).items()):
        if name.startswith("orc_"):
            mine = getattr(L, name)
            mine.restype, mine.argtypes = fn.restype, fn.argtypes
    return L


def first_failure(lib):
    """(case, message) of the first case whose words break a model assertion, or None."""
    rec = HOST.recorded()
    own = LR._lib
    try:
        LR._lib = lib      # (LR.Oracle takes its library from there)
        for case in SC.all_cases():
            frames = HOST.run_oracle(case, lib=lib)
            models = HOST.model_frames(case, [f["vis"] for f in frames])
            prev = None
            for k, (f, m) in enumerate(zip(frames, models)):
                try:
                    HOST.check_words("%s frame %d" % (case.name, SC.FRAMES[k]), f, m, prev, rec["bounds"][case.family])
                except AssertionError as e:
                    return case.name, re.sub(r"\s+", " ", str(e).split(", first")[0])
                prev = f
            if case.sun is not None or case.lights is not None:
                try:
                    HOST.check_direct(case, HOST.run_direct_oracle(case))
                except AssertionError as e:
                    return case.name, re.sub(r"\s+", " ", str(e).split(", first")[0])
    finally:
        LR._lib = own
    return None


def first_path_failure(lib):
    """(run, message) of the first run of path_cases() whose words break the code rule against the model's paths or whose ray count leaves the
    model's, or None."""
    import numpy as np
    for run in SC.path_cases():
        frames = PATHS.run_restatement(run, lib=lib)
        models = PATHS.model_frames(run, [f["vis"] for f in frames])
        prev, bounds = None, PATHS.bounds_of(run)
        for k, f, m in zip(run.positions, frames, models):
            label = "%s frame %d" % (run.name, SC.FRAMES[k])
            try:
                HOST.check_words(label, f, m, prev, bounds)
                flagged = int((m["flags"] != 0).sum())
                assert abs(f["rays"] - m["rays"]) <= 2 * flagged * run.samples * run.depth, "%s: %d rays, the model traces %d" % (label, f["rays"], m["rays"])
            except AssertionError as e:
                return run.name, re.sub(r"\s+", " ", str(e).split(", first")[0])
            prev = f
    return None


def first_hit_failure(lib):
    """(run, message) of the first run of hit_cases() whose words in front of the primary passes break the hit stage's check, or None."""
    for run in SC.hit_cases():
        try:
            PATHS.measure_hits(run, PATHS.run_hit_restatement(run, lib=lib))
        except AssertionError as e:
            return run.name, re.sub(r"\s+", " ", str(e).split(", first")[0])
    return None


def path_main(path):
    lines = ["Mutations of the CPU restatements' path follower and sample loop (the twin lines of raytrace.hip's levels and samples) against the float64",
             "model's paths: the code rule on unflagged pixels and the model's ray count, on the runs of shading_cases.path_cases()",
             "(tests/shading_mutations.py; the unmutated restatement passes every run: tests/test_shading_paths_host.py).", ""]
    with tempfile.TemporaryDirectory() as work:
        clean = first_path_failure(mutated_library([], work))
        assert clean is None, "the unmutated copy fails: %s" % (clean,)
        lines.append("%-48s passes all %d runs" % ("(no mutation)", len(SC.PATH_NAMES)))
        missed = []
        for name, edits, file in PATH_MUTATIONS:
            got = first_path_failure(mutated_library(edits, work, file))
            lines.append("%-48s %s" % (name, "NOT CAUGHT" if got is None else "caught, first by %s" % got[1]))
            if got is None:
                missed.append(name)
        lines += ["", "The sun's and the lights' terms at the hits (tests/light_hit_ref.cpp), judged by the stage check of shading_cases.hit_cases():", ""]
        for name, edits in HIT_MUTATIONS:
            got = first_hit_failure(mutated_library(edits, work, "light_hit_ref.cpp", "light_hit_ref.cpp", LH.lib()))
            lines.append("%-48s %s" % (name, "NOT CAUGHT" if got is None else "caught, first by %s" % got[1]))
            if got is None:
                missed.append(name)
    total = len(PATH_MUTATIONS) + len(HIT_MUTATIONS)
    lines += ["", "%d of %d caught" % (total - len(missed), total)]
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if missed else 0


def main(path):
    lines = ["Mutations of the CPU oracle's shading path (the kernel's twin lines) against the float64 model's code rule on unflagged pixels",
             "(tests/shading_mutations.py; the unmutated oracle passes every case: tests/test_shading_ref_host.py).", ""]
    with tempfile.TemporaryDirectory() as work:
        clean = first_failure(mutated_library([], work))
        assert clean is None, "the unmutated copy fails: %s" % (clean,)
        lines.append("%-40s passes all %d cases" % ("(no mutation)", len(SC.NAMES)))
        missed = []
        for name, edits, *file in MUTATIONS:
            got = first_failure(mutated_library(edits, work, *file))
            lines.append("%-40s %s" % (name, "NOT CAUGHT" if got is None else "caught, first by %s" % got[1]))
            if got is None:
                missed.append(name)
    lines += ["", "%d of %d caught" % (len(MUTATIONS) - len(missed), len(MUTATIONS))]
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if missed else 0


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] not in ("depth1", "paths", "sampled"):
        sys.exit("usage: shading_mutations.py depth1 <report> | paths <report> | sampled <report>")
    sys.exit({"depth1": main, "paths": path_main, "sampled": sampled_main}[sys.argv[1]](sys.argv[2]))
