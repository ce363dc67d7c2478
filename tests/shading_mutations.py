"""Mutation proof of the shading model's assertions, as a host proxy (like profiles/r09_env_mutations.txt): each mutation below is applied to
a scratch copy of the CPU oracle -- the twin line of the kernel's -- which is compiled and put in the kernel's place in the code rule of
tests/test_shading_ref_host.py (check_words against the float64 model on unflagged pixels, the GPU test's own assertion).  Bit equality with
itself would pass every one of them; a mutation no case catches means a missing case.  Run by hand, it writes the report:

    python tests/shading_mutations.py profiles/r20_shading_mutations.txt

The last two are lines of the sun's and the lights' restatements (tests/sun_ref.cpp, tests/lights_ref.cpp) and are judged by the stage check
of those passes (check_direct)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

import lights_ref as LR
import restatement as RS
import shading_cases as SC
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


def mutated_library(edits, work, file=None):
    """The whole oracle and every restatement (tests/lights_ref.cpp includes them all) from a scratch copy with the edits applied."""
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
    subprocess.check_call([os.environ.get("CXX", "g++")] + RS._FLAGS + ["-shared", "-pthread", "-o", out, os.path.join(work, "tests", "lights_ref.cpp")])
    L = C.CDLL(out)
    for name, fn in list(vars(LR.lib()).items()):
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
    sys.exit(main(sys.argv[1]))
