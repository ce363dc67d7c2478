"""GGX-prefiltered environments without a GPU (rtggx_prefilter_env): the host's sample tables (raytracedggx_amd/csrc/rt_env_filter.h, printed
by the stand-alone tests/env_filter_main.cpp, also under AddressSanitizer and UBSan) against the restatement tests/envfilter_ref.cpp bit for
bit and against a numpy float64 evaluation of the contract's formulas; the restatement itself on constant cubes and against a float64 model
of the same sum; the executable's flag; the declaration, the export and the binding."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import assets
import env_cases as EC
import envfilter_ref as F
import envimage_ref as E
import host_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES, COUNTS = (1, 5, 16, 33, 64, 256), (64, 256, 4096)
EPS = 2.0 ** -24


# ---- 1. the table of rt_env_filter.h ---------------------------------------------------------------------------------------------------
def compile_main(exe, sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to build the stand-alone program with")
    flags = ["-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-fast-math"]
    flags += ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    r = subprocess.run([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "env_filter_main.cpp")], capture_output=True, text=True)
    if sanitize and r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b|unrecognized (command[- ]line )?option .*-fsanitize", r.stderr):
        pytest.skip("the sanitizer runtime is missing: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    return exe


def run_tables(exe, pairs):
    """-> {(S, N, m): (float32 [K, 4], invW as float32, M)} from the program's binary output."""
    r = subprocess.run([exe, "tables"] + [str(v) for p in pairs for v in p], capture_output=True, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err
    words, at, out = np.frombuffer(r.stdout, np.uint32), 0, {}
    while at < words.size:
        S, M, m, N, K, inv = (int(v) for v in words[at:at + 6]); at += 6
        out[(S, N, m)] = (words[at:at + 4 * K].view(np.float32).reshape(K, 4), np.array([inv], np.uint32).view(np.float32)[0], M); at += 4 * K
    assert at == words.size
    return out


@pytest.fixture(scope="module")
def header_tables(tmp_path_factory):
    exe = compile_main(str(tmp_path_factory.mktemp("envfilter") / "env_filter_main"), sanitize=False)
    return run_tables(exe, [(S, N) for S in SIDES for N in COUNTS])


def test_header_tables_equal_the_restatement_bit_for_bit(header_tables):
    """Every level of every (S, N): K, the entries and invW.  A side of 1 has no level below level 0 and no table."""
    assert sorted(header_tables) == sorted((S, N, m) for S in SIDES for N in COUNTS for m in range(1, F.levels_of(S)))
    for (S, N, m), (t, inv, M) in header_tables.items():
        assert M == F.levels_of(S)
        want, want_inv = F.table(S, M, m, N)
        assert t.shape == want.shape, (S, N, m, t.shape, want.shape)
        np.testing.assert_array_equal(t.view(np.uint32), want.view(np.uint32), err_msg="S %d N %d level %d" % (S, N, m))
        assert inv.view(np.uint32) == want_inv.view(np.uint32), (S, N, m, inv, want_inv)


def test_header_tables_have_the_contracts_properties(header_tables):
    """K = N / 2 on every level of roughness 1 (m >= M - 4: the even i) and N / 2 < K <= N below; entry 0 is (0, 0, 1, .); z in (0, 1]; unit
    length to 4 x 2^-24 (three components rounded to fp32, 2^-24 relative each, enter the squared length twice); lod in [0, M - 1]; invW the
    rounded reciprocal of the sum of z; every entry within one fp32 ulp of the float64 evaluation of the same formulas in numpy."""
    for (S, N, m), (t, inv, M) in header_tables.items():
        label = "S %d N %d level %d" % (S, N, m)
        K = t.shape[0]
        if m >= M - 4:
            assert F.roughness(m, M) == 1.0 and K == N // 2, label
        else:
            assert F.roughness(m, M) < 1.0 and N // 2 < K <= N, label
        assert t[0, 0] == 0.0 and t[0, 1] == 0.0 and t[0, 2] == 1.0, label
        d = t.astype(np.float64)
        assert (d[:, 2] > 0.0).all() and (d[:, 2] <= 1.0).all(), label
        assert np.abs((d[:, :3] ** 2).sum(axis=1) - 1.0).max() <= 4.0 * EPS, label
        assert (d[:, 3] >= 0.0).all() and (d[:, 3] <= M - 1).all(), label
        assert np.float32(1.0 / d[:, 2].sum()) == inv, label      # (numpy adds pairwise: the sums agree far inside an fp32 rounding, or this would tell)
        kept, want = F.table_float64(S, M, m, N)
        assert kept.shape[0] == K and kept[0] == 0, label
        if m >= M - 4:
            np.testing.assert_array_equal(kept, np.arange(0, N, 2), err_msg=label)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(d - want) <= ulp).all(), "%s: entry %d is %r, float64 %r" % (label, (np.abs(d - want) / ulp).max(axis=1).argmax(), t[(np.abs(d - want) / ulp).max(axis=1).argmax()], want[(np.abs(d - want) / ulp).max(axis=1).argmax()])


def test_env_filter_header_under_address_and_undefined_behaviour_sanitizers(tmp_path, header_tables):
    """The same program built with -fsanitize=address,undefined and run on its own (the runtimes are linked in: nothing is preloaded and
    nothing is loaded into Python): it ends clean and prints the tables of the plain build; the argument check's answers."""
    exe = compile_main(str(tmp_path / "env_filter_main_san"), sanitize=True)
    pairs = [(1, 64), (5, 64), (33, 256), (64, 4096)]
    got = run_tables(exe, pairs)
    assert sorted(got) == sorted(k for k in header_tables if (k[0], k[1]) in pairs)
    for k, (t, inv, M) in got.items():
        np.testing.assert_array_equal(t.view(np.uint32), header_tables[k][0].view(np.uint32))
        assert inv == header_tables[k][1] and M == header_tables[k][2]
    values = [0, 1, 32, 48, 63, 64, 65, 100, 128, 256, 512, 1024, 2048, 4096, 4097, 8192, 0x80000000, 0xFFFFFFFF]
    r = subprocess.run([exe, "samples"] + [str(v) for v in values], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    accepted = {0: 1024, 64: 64, 128: 128, 256: 256, 512: 512, 1024: 1024, 2048: 2048, 4096: 4096}
    assert [tuple(int(w) for w in l.split()) for l in r.stdout.splitlines()] == [(v, 1 if v in accepted else 0, accepted.get(v, 0)) for v in values]


# ---- 2. the restatement ------------------------------------------------------------------------------------------------------------------
def half_spacing(c):
    return 2.0 ** (np.floor(np.log2(c)) - 10.0)


@pytest.mark.parametrize("value", [1.0, 1000.0])
@pytest.mark.parametrize("size, samples", [(5, 64), (16, 256), (33, 64)])
def test_restatement_keeps_a_constant_cube_constant(size, samples, value):
    """Every texel of every level is the constant to within one binary16 spacing: the box chain below a constant level 0 is the constant to
    a few fp32 roundings, every tap returns it to a few more, the terms z_k c are non-negative -- so the sum over ceil(K / 64) terms per
    partial and six levels of the tree is (sum of z) c to (ceil(K / 64) + 8) 2^-24 relative, and times invW the constant again, far below
    the half rounding."""
    cube = EC.constant_cube(size, value)
    got = F.prefilter(cube.codes[0], samples, threads=4)
    assert got.shape[0] == 6 * sum(s * s for s in E.chain_sides(size))
    v = got[:, :3].copy().view(np.float16).astype(np.float64)
    assert np.abs(v - value).max() <= half_spacing(value), (size, samples, value, v.min(), v.max())
    assert (got[6 * size * size:, 3] == 0x3C00).all()      # alpha 1 below level 0 (constant_cube's own alpha is the constant)
    np.testing.assert_array_equal(got[:6 * size * size], cube.codes[0].reshape(-1, 4))      # level 0 bit for bit


@pytest.mark.parametrize("size, samples", [(16, 256), (33, 64)])
def test_restatement_lies_within_the_derived_bound_of_the_float64_model(size, samples):
    """On env_cases.random_cube: per texel and component |restatement - model| <= sum_k z_k bound(C, lod_k) invW (the sampler's per-tap
    bound of tests/env_cases.py, summed with the weights) + (K + 8) 2^-24 value (the fp32 sum of non-negative terms and the scaling) + the
    half rounding of the value.  The model takes the contract's fp32 directions and table entries as they are and evaluates the taps with
    tests/env_ref.py's float64 sampler, accumulating in double; where a corner tap takes part it gives an interval, and the restatement
    must lie within the bound of it."""
    level0 = EC.random_cube(size, 1).codes[0]
    M = F.levels_of(size)
    src = F.source_cube(level0)
    sides = E.chain_sides(size)
    codes, at = [], 0
    for s in sides:
        codes.append(src[at:at + 6 * s * s].reshape(6, s, s, 4)); at += 6 * s * s
    C = EC.Cube(size, M, codes, "C_%d" % size)
    got = E.unpack(F.prefilter(level0, samples, threads=4), size)
    tables, inv = {}, {}
    for m in range(1, M):
        tables[m], inv[m] = F.table(size, M, m, samples)
    model = F.model(C.levels, size, tables, inv)
    worst = 0.0
    for m in range(1, M):
        t = tables[m].astype(np.float64)
        K = t.shape[0]
        lo, hi = model[m]
        taps = float((t[:, 2] * EC.bound(C, t[:, 3])).sum() * float(inv[m]))
        tol = taps + (K + 8) * EPS * hi + E.half_rounding(hi)
        over = np.maximum(lo - got[m], got[m] - hi)      # <= 0 inside the interval
        print("side %d N %d level %d: K %d, largest excess / bound = %.4f (taps' part of the bound %.3e)" % (size, samples, m, K, (over / tol).max(), taps))
        worst = max(worst, float((over / tol).max()))
        assert (over <= tol).all(), "side %d level %d: texel %d is %.3f bounds from the model" % (size, m, (over / tol).argmax(), (over / tol).max())
        assert hi.max() > 1.0      # (a cube of radiance in [0, 8): the levels are not black)
    assert worst <= 1.0


# ---- 3. the executable and the C ABI ---------------------------------------------------------------------------------------------------
def test_executable_refuses_a_bad_sample_count_before_it_asks_for_a_device(built):
    env = ["-env", assets.path("rnl_cross.dds")]
    host_support.executable_refuses([env + ["-envprefilter", "100"], env + ["-envprefilter", "32"], env + ["-envprefilter", "8192"],
                                     env + ["-envprefilter", "0"], env + ["-envprefilter", "64x"], ["-envprefilter", "-1"] + env],
                                    must_mention="-envprefilter", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


def test_executable_parses_envprefilter_with_and_without_a_number(built, tmp_path):
    """-envprefilter alone (1024), followed by another flag, and with a good number: the command line parses -- what stops these runs is the
    environment file, which is read after the command line and before a device is asked for."""
    missing = str(tmp_path / "missing.hdr")
    host_support.executable_refuses([["-envprefilter", "-env", missing], ["-env", missing, "-envprefilter"], ["-envprefilter", "64", "-env", missing],
                                     ["-env", missing, "-envprefilter", "4096", "-envmips"], ["/envprefilter", "/env", missing]],
                                    must_mention="cannot open", scene=("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64"))


def test_c_abi_and_host_declare_the_new_entry_point(built):
    host_support.declared_exported_bound("rtggx_prefilter_env", r"int\s+rtggx_prefilter_env\(rtggx_context\* ctx, uint32_t samples\);",
                                         defines=(r"#define RTGGX_ENV_FILTER_MIN_SAMPLES 64u", r"#define RTGGX_ENV_FILTER_MAX_SAMPLES 4096u"))
    from raytracedggx_amd import capi
    assert (capi.ENV_FILTER_MIN_SAMPLES, capi.ENV_FILTER_MAX_SAMPLES) == (F.MIN_SAMPLES, F.MAX_SAMPLES) == (64, 4096)
    with open(os.path.join(ROOT, "raytracedggx_amd", "csrc", "rt_env_filter.h")) as f:
        header = f.read()
    assert "hip" not in " ".join(re.findall(r"^\s*#\s*include\s*(\S+)", header, re.M)).lower()      # the table's header holds no device code
    with open(os.path.join(ROOT, "tests", "envfilter_ref.cpp")) as f:
        assert "rt_env_filter.h\"" not in "".join(l for l in f if l.lstrip().startswith("#"))      # the restatement does not include it
