"""The host's argument for leaving still and settled sky alone (raytracedggx_amd/csrc/rt_sky_chain.h), without a GPU: the header includes
nothing of HIP, so tests/sky_chain_main.cpp -- a program of its own that drives a SkyChain through scripted frame sequences -- is built
with a host compiler under AddressSanitizer and UBSan and run as a child process.  The runtimes are linked into the program
(-static-libasan): nothing is preloaded and nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracedggx_amd", "csrc")


def test_sky_chain_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Every decision of every scripted frame is the one written out in sky_chain_main.cpp, beside the sentence of the header it follows
    from: the steady state, each event that starts a new epoch and the recovery from it, the chains that break without one (a visibility
    pass alone, no denoiser, a fused pass, another source, an empty strip, other images, a narrow frame, the switches), the stale-history
    guard on its own, and the epoch's wrap.  The program must end clean, without a word from either sanitizer."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to build the stand-alone program with")
    exe = str(tmp_path / "sky_chain")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "sky_chain_main.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b|unrecognized (command[- ]line )?option .*-fsanitize", r.stderr):
        pytest.skip("the sanitizer runtime is missing: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr)
    assert re.search(r"sky chain: all \d+ checks passed", r.stdout), r.stdout


def test_the_sky_chain_header_is_free_of_hip_and_the_launchers_of_its_rules():
    """rt_sky_chain.h includes <cstdint> and <cstring> alone; no other file of csrc spells a rule out again or ends the runs without a reason."""
    with open(os.path.join(CSRC, "rt_sky_chain.h")) as f:
        header = f.read()
    assert sorted(re.findall(r"^\s*#\s*include\s*(\S+)", header, re.M)) == ["<cstdint>", "<cstring>"]
    old = re.compile(r"genValid|SkyTM|SkyV\b|skyEpochForGen|MaySkip|breakSkyRuns")
    bare = re.compile(r"breakRuns\(\s*\)")
    found = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "rt_sky_chain.h":
            with open(os.path.join(CSRC, name)) as f:
                for k, line in enumerate(f, 1):
                    if old.search(line) or bare.search(line) or ("breakRuns(" in line and "SkyBreak::" not in line):
                        found.append("%s:%d: %s" % (name, k, line.strip()[:100]))
    assert not found, "\n".join(found)
