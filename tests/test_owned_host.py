"""The owner template behind every device buffer, event and stream of librtggx (raytracedggx_amd/csrc/rt_owned.h), without a GPU: its
generic part includes nothing of HIP, so tests/owned_main.cpp -- a program of its own with a counting release functor -- is built with a
host compiler under AddressSanitizer and UBSan and run as a child process.  The runtimes are linked into the program (-static-libasan):
nothing is preloaded and nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Moves leave the source empty and release the overwritten value exactly once; reset / release / put() release or do not, as
    rt_owned.h says; a self-move-assignment releases nothing; the destructor releases once and an empty owner never calls the functor;
    an array of owners with only entry 0 filled releases once.  The program must end clean, without a word from either sanitizer."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to build the stand-alone program with")
    exe = str(tmp_path / "owned")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-self-move", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "owned_main.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b|unrecognized (command[- ]line )?option .*-fsanitize", r.stderr):
        pytest.skip("the sanitizer runtime is missing: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr)
    assert "owned: all checks passed" in r.stdout, r.stdout


def test_only_the_owner_header_calls_the_runtimes_release_functions():
    """The end state the owners exist for: in csrc, hipFree / hipHostFree / hipEventDestroy / hipStreamDestroy / hipIpcCloseMemHandle are
    called by rt_owned_hip.h alone, and the matching allocation and creation functions only there as well."""
    csrc = os.path.join(ROOT, "raytracedggx_amd", "csrc")
    words = re.compile(r"\b(hipFree|hipHostFree|hipEventDestroy|hipStreamDestroy|hipIpcCloseMemHandle|hipMalloc|hipHostMalloc|hipEventCreate\w*|hipStreamCreate\w*)\s*\(")
    found = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")) and name != "rt_owned_hip.h":
            with open(os.path.join(csrc, name)) as f:
                for k, line in enumerate(f, 1):
                    code = line.split("//")[0]
                    if words.search(code):
                        found.append("%s:%d: %s" % (name, k, code.strip()[:100]))
    assert not found, "\n".join(found)
