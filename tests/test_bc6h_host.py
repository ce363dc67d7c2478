"""BC6H without a GPU: the oracle's decoder (oracle/orc_dds.h, the kernel's twin) against the exact-integer model of tests/bc6h_cases.py, both
against a decoder that shares no text with the project (Pillow, recorded in tests/golden/bc6h_pillow.npz by tests/golden/make_bc6h_golden.py),
and the host's container reader (host/DDSLoader.h) as a stand-alone program, plain and under AddressSanitizer and UBSan, over well-formed and
malformed files.

Pillow shows 8 bits per channel; a half h is taken to 8 bits as Pillow does: below 0 -> 0, above 1 -> 255, else int(float32(h) * 255).  Under
that rule the model differs from Pillow by at most 1, and only upward, and only in the modes whose endpoints are wider than 10 bits.  The whole
remainder is one term: with the interpolation's "+ 32" left out, the model equals Pillow on every channel of the fixture.  The format's
text has the term (v = (a (64 - w) + b w + 32) >> 6, Direct3D 11 "BC6H format" and the Khronos Data Format Specification alike), so the
model, the oracle and the kernel keep it.  Up to 10 bits the unquantized endpoints are multiples of 64, or all 32 above one (0xFFFF
aside): the weighted sum is a multiple of 64, the term changes nothing, and those modes agree exactly.  Above 10 bits half of the sums
change, 31/64 of those move the half by one step, and a half's step is 1/8 ... 1/32 of an 8-bit step in [1/8, 1): about 2 % of the
channels in that range, fewer below it, none outside (0, 1).

What is asserted, per mode and format:
  * the model without the term equals Pillow, channel for channel, on the whole fixture (the share of differing channels is 0);
  * the format's model, and the oracle, are never below Pillow and never more than 1 above, on the whole fixture;
  * on the fixture's random blocks, at most 1 % of a mode's channels are off by one (measured: 0.2 % at most).  Over the crafted blocks and the
    single-bit flips, nearly all of whose channels lie in [1/8, 1], the share is what the arithmetic above says, up to 4.2 % in modes 0x0b and
    0x0f; it is printed, and the first assertion holds those blocks to more than a share would;
  * the oracle equals the format's model, bit for bit, on every fixture block.

profiles/r25_bc6h_mutations.txt records which of these legs catches each of a list of single-token mutations of the oracle."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import assets
import bc6h_cases as BC
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_SHARE = 0.01            # of the channels of one mode and format that may be off by one


def oracle_decode(blocks, signed):
    return np.stack([O.bc6h_decode_block(b.tobytes(), signed=signed) for b in blocks])


# ---- the table and the model by themselves -------------------------------------------------------------------------------------------
def test_layout_table_gives_every_position_one_meaning():
    """Each mode: the mode bits, the field bits and the index bits tile the 128 positions exactly, whatever the partition; each field has
    the width the mode's endpoint and delta widths call for."""
    for mid, md in BC.MODES.items():
        for d in (range(32) if md.regions == 2 else (0,)):
            first, widths = BC.index_layout(md, d)
            seen = list(range(md.mode_bits)) + [p for f in BC.FIELDS + ("d",) for p in md.pos[f]] + list(range(first, first + sum(widths)))
            assert sorted(seen) == list(range(128)), "mode %#x partition %d" % (mid, d)
        for c, ch in enumerate("rgb"):
            assert len(md.pos[ch + "w"]) == md.wbits
            assert len(md.pos[ch + "x"]) == md.delta[c]
            assert len(md.pos[ch + "y"]) == len(md.pos[ch + "z"]) == (md.delta[c] if md.regions == 2 else 0)
    for d in range(32):
        assert not BC.PARTITION[d] & 1 and (BC.PARTITION[d] >> BC.ANCHOR[d]) & 1          # texel 0 anchors region 0, ANCHOR[d] lies in region 1
    for n, w in BC.WEIGHTS.items():
        assert len(w) == 1 << n and all(w[i] + w[-1 - i] == 64 for i in range(len(w)))


def test_assemble_and_parse_are_inverse_and_the_cases_are_what_they_claim():
    names, blocks = BC.all_cases()
    assert len(set(names)) == len(names) == len(blocks)
    for name, blk in zip(names, blocks):
        mid, fields, d, idx = BC.parse(blk)
        if mid is not None:
            assert BC.assemble(mid, fields, d, idx) == blk.tobytes(), name
    count = lambda pat: sum(1 for n in names if re.search(pat, n))
    for mid in BC.MODE_IDS:
        md = BC.MODES[mid]
        assert count(r"^mode %#04x random" % mid) == BC.N_RANDOM
        assert count(r"^mode %#04x partition" % mid) == (32 if md.regions == 2 else 0)
        # every index value at every texel, per partition tried
        for d in ((0, 17, 18) if md.regions == 2 else (0,)):
            seen = [set() for _ in range(16)]
            for name, blk in zip(names, blocks):
                if name.startswith("mode %#04x indices d%d " % (mid, d)):
                    for i, v in enumerate(BC.parse(blk)[3]):
                        seen[i].add(v)
            widths = BC.index_layout(md, d)[1]
            assert [len(s) for s in seen] == [1 << w for w in widths], (mid, d)
        # the special endpoints and both directions of wrap occur, per channel
        ws = {ch: set() for ch in "rgb"}
        wraps = {(ch, up): 0 for ch in "rgb" for up in (0, 1)}
        for name, blk in zip(names, blocks):
            if name.startswith("mode %#04x " % mid) and " random " not in name:
                _, f, _, _ = BC.parse(blk)
                for c, ch in enumerate("rgb"):
                    ws[ch].add(f[ch + "w"])
                    if md.transformed:
                        for e in "xyz"[:3 if md.regions == 2 else 1]:
                            s = f[ch + "w"] + BC.sign_extend(f[ch + e], md.delta[c])
                            wraps[(ch, 1)] += s >= 1 << md.wbits
                            wraps[(ch, 0)] += s < 0
        top, half = (1 << md.wbits) - 1, 1 << (md.wbits - 1)
        for ch in "rgb":
            assert {0, 1, top, top - 1, half, half + 1, half - 1} <= ws[ch], (mid, ch)
            assert not md.transformed or (wraps[(ch, 0)] >= 3 and wraps[(ch, 1)] >= 3), (mid, ch, wraps)
    for id5 in range(32):
        assert count(r"^id %#04x random" % id5) == 8


def test_model_known_answers():
    """The model against arithmetic done by hand on the rules, with no code shared: the special values of both unquantize rules, the floor
    shift, the finish, a wrap in each direction, an anchor's short index, a reserved id."""
    assert [BC.unquantize(e, 10, False) for e in (0, 1, 1022, 1023)] == [0, 96, 65440, 0xFFFF]            # (1 << 16) + 0x8000 >> 10 = 96
    assert BC.unquantize(0xFFFE, 16, False) == 0xFFFE and BC.unquantize(-0x8000, 16, True) == -0x8000
    assert [BC.unquantize(e, 10, True) for e in (0, 1, -1, 510, 511, -511, -512)] == [0, 96, -96, 32672, 0x7FFF, -0x7FFF, -0x7FFF]
    assert BC.finish(0xFFFF, False) == 0x7BFF and BC.finish(0x7FFF, True) == 0x7BFF and BC.finish(-0x7FFF, True) == 0xFBFF and BC.finish(-1, True) == 0x8000
    # mode 0x02 (11 bits; deltas 5, 4, 4): red wraps upward 2047 + 2 -> 1, green downward 0 - 1 -> 2047, blue stays: 1000 + 7
    f = dict(rw=2047, rx=2, gw=0, gx=0xF, bw=1000, bx=7, ry=0, rz=0, gy=0, gz=0, by=0, bz=0)
    e = BC.endpoints(0x02, f, False)
    assert e[0][1] == [1, 2047, 1007] and e[0][0] == [2047, 0, 1000]
    assert BC.endpoints(0x02, f, True)[0] == [[-1, 0, 1000], [1, -1, 1007]]
    # interpolation with a floor shift on negatives: a = -96, b = 0; weight 4: (-96 * 60 + 32) / 64 = -89.5 -> -90; weight 0: -95.5 -> -96
    out = BC.decode_fields(0x03, dict(rw=-1 & 1023, rx=0, gw=0, gx=0, bw=0, bx=0, ry=0, rz=0, gy=0, gz=0, by=0, bz=0), 0, [1] + [0] * 15, True)
    assert out[0][0] == 0x8000 | ((90 * 31) >> 5) and out[1][0] == 0x8000 | ((96 * 31) >> 5)
    # partition 17 = 0x008E: texels 1, 2, 3 and 7 are region 1, the anchor is texel 2 (2 bits); index bits start at 82
    blk = BC.assemble(0x1e, dict(rw=10, rx=20, ry=40, rz=50, gw=0, gx=0, gy=0, gz=0, bw=0, bx=0, by=0, bz=0), 17, [3, 7, 3, 0] + [0] * 12)
    acc = int.from_bytes(blk, "little")
    assert (acc >> 82) & 0x3 == 3 and (acc >> 84) & 0x7 == 7 and (acc >> 87) & 0x3 == 3 and acc >> 89 == 0
    got = BC.decode_block(blk, False)[:, 0]
    unq = lambda c: ((c << 16) + 0x8000) >> 6
    lerp = lambda a, b, w: (((unq(a) * (64 - w) + unq(b) * w + 32) >> 6) * 31) >> 6
    assert list(got[:4]) == [lerp(10, 20, 27), lerp(40, 50, 64), lerp(40, 50, 27), lerp(40, 50, 0)] and got[4] == lerp(10, 20, 0) and got[7] == lerp(40, 50, 0)
    assert not BC.decode_block(bytes([0xF3] + [0xFF] * 15), False).any()


# ---- the oracle against the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [False, True], ids=["UF16", "SF16"])
def test_oracle_equals_the_model_on_every_case(built, signed):
    names, blocks = BC.all_cases()
    got, want = oracle_decode(blocks, signed), BC.expected(signed)
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, "%d of %d cases differ, first: %s block %s: oracle %s, model %s" % (
        bad.size, len(names), names[bad[0]], blocks[bad[0]].tobytes().hex(), got[bad[0]].tolist(), want[bad[0]].tolist())
    for id5 in BC.RESERVED:
        at = [i for i, n in enumerate(names) if n.startswith("id %#04x" % id5)]
        assert len(at) == 9 and not got[at].any()


# ---- both against Pillow ---------------------------------------------------------------------------------------------------------------
def load_golden():
    g = np.load(os.path.join(HERE, "golden", "bc6h_pillow.npz"))
    out = {"version": str(g["pillow_version"]), "formats": [int(v) for v in g["formats"]], "mode_ids": [int(v) for v in g["mode_ids"]]}
    for key in ("uf16", "sf16"):
        blocks, pos = g["blocks_" + key], g["flip_pos_" + key].astype(np.int64)
        flipped = blocks[g["flip_base_" + key]].copy()
        flipped[np.arange(len(flipped)), pos >> 3] ^= (1 << (pos & 7)).astype(np.uint8)
        out[key] = dict(blocks=np.concatenate([blocks, flipped]), pillow=np.concatenate([g["pillow_" + key], g["pillow_flip_" + key]]),
                        stored=len(blocks), flip_base=g["flip_base_" + key].astype(np.int64), kind=np.concatenate([g["kind_" + key], np.full(len(flipped), 3, np.uint8)]), witnessed=g["witnessed_" + key], left_out=[int(v) for v in g[key + "_left_out"]])
    return out


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def shares(ours8, pillow, blocks, what):
    """Per mode: (channels, off by one, largest difference, smallest signed difference); prints them."""
    modes = np.array([BC.mode_of(b) for b in blocks])
    out = {}
    for mid in BC.MODE_IDS:
        at = modes == mid
        if not at.any():
            continue
        d = ours8[at].astype(np.int64) - pillow[at].astype(np.int64)
        out[mid] = (d.size, int((d != 0).sum()), int(np.abs(d).max()), int(d.min()))
        print("%s mode %#04x: %d of %d channels differ from Pillow (%.3f %%), by at most %d" % (what, mid, out[mid][1], d.size, 100.0 * out[mid][1] / d.size, out[mid][2]))
    return out


@pytest.mark.parametrize("key", ["uf16", "sf16"])
def test_model_against_pillow(golden, key):
    g, signed = golden[key], key == "sf16"
    assert golden["formats"] == [95, 96] and golden["mode_ids"] == list(BC.MODE_IDS)
    print("Pillow %s, %s: %d stored blocks and %d single-bit flips of them" % (golden["version"], key, g["stored"], len(g["blocks"]) - g["stored"]))
    # every mode is there, none left out; SF16: the nine transformed modes below 16 bits only with non-negative endpoints and no wrap
    assert g["left_out"] == [] and sorted(set(BC.mode_of(b) for b in g["blocks"])) == sorted(BC.MODE_IDS)
    if signed:
        for blk in g["blocks"]:
            mid, f, _, _ = BC.parse(blk)
            md = BC.MODES[mid]
            if mid in (0x1e, 0x03, 0x0f):
                continue
            for c, ch in enumerate("rgb"):
                ends = [f[ch + "w"]] + [f[ch + "w"] + BC.sign_extend(f[ch + e], md.delta[c]) for e in "xyz"[:3 if md.regions == 2 else 1]]
                assert all(0 <= v < 1 << (md.wbits - 1) for v in ends), "an SF16 block of mode %#x outside what Pillow is trusted on" % mid
    # the model without the interpolation's + 32: Pillow, channel for channel
    np.testing.assert_array_equal(BC.half_to_8bit(BC.decode_blocks(g["blocks"], signed, rounding=0)), g["pillow"])
    check_against_pillow(BC.half_to_8bit(BC.decode_blocks(g["blocks"], signed)), g, key + " model")


def check_against_pillow(ours8, g, what):
    """The format's decode (with the rounding term) against Pillow's (without): never below, at most 1 above; on the random blocks at most 1 % of
    a mode's channels off by one."""
    for mid, (n, off, worst, low) in shares(ours8, g["pillow"], g["blocks"], what + ", whole fixture,").items():
        assert worst <= 1 and low >= 0, (what, hex(mid), n, off, worst, low)
    rnd = np.nonzero(g["kind"] == 2)[0]
    assert 2 * len(rnd) >= g["stored"]          # the random blocks are the larger half of what is stored
    for mid, (n, off, worst, low) in shares(ours8[rnd], g["pillow"][rnd], g["blocks"][rnd], what + ", random blocks,").items():
        assert off <= MAX_SHARE * n, (what, hex(mid), n, off, worst, low)


@pytest.mark.parametrize("key", ["uf16", "sf16"])
def test_oracle_against_pillow(built, golden, key):
    g, signed = golden[key], key == "sf16"
    got = oracle_decode(g["blocks"], signed)
    check_against_pillow(BC.half_to_8bit(got), g, key + " oracle")
    np.testing.assert_array_equal(got, BC.decode_blocks(g["blocks"], signed))


@pytest.mark.parametrize("key", ["uf16", "sf16"])
def test_pillow_saw_every_bit(golden, key):
    """A golden proves only what it can see.  Per mode, the positions p after the mode bits for which the fixture's maker found a stored block
    B with Pillow(B) != Pillow(B ^ (1 << p)).  Allowed to be missing: the lowest four endpoint bits of modes 0x0b and 0x0f, where a step is
    below what 8 bits resolve (no layout leaves a position unused).  Most flips are stored; those the models must reproduce: the block
    and its flip differ in the model's 8-bit answer as well."""
    g, signed = golden[key], key == "sf16"
    for mi, mid in enumerate(BC.MODE_IDS):
        md = BC.MODES[mid]
        mask = int.from_bytes(g["witnessed"][mi].tobytes(), "little")
        print("%s mode %#04x witnessed %032x" % (key, mid, mask))
        assert mask & ((1 << md.mode_bits) - 1) == 0
        allowed = {p for f in ("rw", "gw", "bw") for p in md.pos[f][:4]} if mid in (0x0b, 0x0f) else set()
        missing = {p for p in range(md.mode_bits, 128) if not (mask >> p) & 1}
        assert missing <= allowed, "%s mode %#x: Pillow never saw positions %s" % (key, mid, sorted(missing - allowed))
    n = g["stored"]
    flips, base = g["blocks"][n:], g["pillow"]
    ours = BC.half_to_8bit(BC.decode_blocks(g["blocks"], signed, rounding=0))
    src = g["flip_base"]
    assert (base[n:] != base[src]).any(axis=(1, 2)).all() and (ours[n:] != ours[src]).any(axis=(1, 2)).all()
    assert len(flips) >= 0.9 * sum(128 - BC.MODES[m].mode_bits for m in BC.MODE_IDS)


# ---- the container reader as a stand-alone program -------------------------------------------------------------------------------------
def compile_main(exe, sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to build the stand-alone program with")
    flags = ["-std=c++17", "-g", "-Wall", "-Wextra"]
    flags += ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else ["-O2"]
    r = subprocess.run([gxx] + flags + ["-o", exe, os.path.join(HERE, "dds_loader_main.cpp")], capture_output=True, text=True)
    if sanitize and r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b|unrecognized (command[- ]line )?option .*-fsanitize", r.stderr):
        pytest.skip("the sanitizer runtime is missing: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    return exe


def payload_bytes(fmt, size, mips):
    side = lambda m: max(size >> m, 1)
    return 6 * sum(((side(m) + 3) // 4) ** 2 * 16 if fmt in (95, 96) else side(m) ** 2 * (8 if fmt == 10 else 16) for m in range(mips))


def dds_file(width, mips, fmt=None, payload=b"", height=None, magic=b"DDS ", header_size=124, pf_size=32, pf_flags=0x4, fourcc=b"DX10", caps2=0, misc=0x4):
    """A DDS file: the 128-byte header, the 20-byte DX10 header where fmt is given, the payload."""
    fourcc = fourcc if isinstance(fourcc, bytes) else struct.pack("<I", fourcc)
    head = magic + struct.pack("<7I", header_size, 0x1 | 0x2 | 0x4 | 0x1000 | 0x20000, width if height is None else height, width, 0, 0, mips) + bytes(44)
    head += struct.pack("<II", pf_size, pf_flags) + fourcc + bytes(20) + struct.pack("<5I", 0x1008, caps2, 0, 0, 0)
    assert len(head) == 128
    return head + (struct.pack("<5I", fmt, 3, misc, 1, 0) if fmt is not None else b"") + payload


def loader_files():
    """-> [(name, bytes, expected line after 'name: ')]."""
    rng = np.random.default_rng(0xDD5)
    files = []

    def good(name, size, mips, fmt, header_mips=None, **kw):
        dxgi = fmt if kw.get("fourcc", b"DX10") == b"DX10" else None
        body = rng.integers(0, 256, payload_bytes(fmt, size, mips), dtype=np.uint8).tobytes()
        files.append((name, dds_file(size, mips if header_mips is None else header_mips, dxgi, body + b"trailing bytes are not payload", **kw),
                      "format %d size %d mips %d bytes %d fnv %08x" % (fmt, size, mips, len(body), assets.fnv1a32(body))))

    def bad(name, data, error):
        files.append((name, data, "error: " + error))

    for fmt in (95, 96, 10, 2):                                       # all four formats, every small side, with and without a chain
        for size in (1, 2, 3, 4, 5):
            good("f%d_s%d_m1" % (fmt, size), size, 1, fmt)
            full = size.bit_length()
            if full > 1:
                good("f%d_s%d_full" % (fmt, size), size, full, fmt)
    good("mips0_reads_as_1", 4, 1, 95, header_mips=0)
    good("s16_full", 16, 5, 96)
    good("s12_m3", 12, 3, 95)
    good("legacy113", 3, 2, 10, fourcc=113, caps2=0x200)
    good("legacy116", 2, 2, 2, fourcc=116, caps2=0x200)
    good("cube_by_caps2_only", 4, 3, 95, caps2=0x200, misc=0)
    whole = dds_file(8, 4, 95, rng.integers(0, 256, payload_bytes(95, 8, 4), dtype=np.uint8).tobytes())
    bad("len0", b"", "not a DDS file")
    bad("len3", whole[:3], "not a DDS file")
    bad("len127", whole[:127], "not a DDS file")
    bad("len128_dx10", whole[:128], "truncated DX10 header")
    bad("len147", whole[:147], "truncated DX10 header")
    bad("len148", whole[:148], "truncated payload")
    bad("one_byte_short", whole[:-1], "truncated payload")
    for fmt in (95, 10, 2):
        bad("s8192_f%d_header_only" % fmt, dds_file(8192, 14, fmt, bytes(1000)), "truncated payload")
    bad("legacy113_short", dds_file(4, 1, None, bytes(6 * 4 * 4 * 8 - 1), fourcc=113, caps2=0x200), "truncated payload")
    body = bytes(payload_bytes(95, 8, 4))
    bad("wrong_magic", dds_file(8, 4, 95, body, magic=b"DDS\0"), "not a DDS file")
    bad("wrong_header_size", dds_file(8, 4, 95, body, header_size=128), "not a DDS file")
    bad("wrong_pf_size", dds_file(8, 4, 95, body, pf_size=0), "not a DDS file")
    bad("no_fourcc_flag", dds_file(8, 4, 95, body, pf_flags=0x40), "unsupported DDS pixel format")
    bad("unknown_fourcc", dds_file(8, 4, None, body, fourcc=b"DXT5", caps2=0x200), "unsupported DDS pixel format")
    bad("no_cube_flag", dds_file(8, 4, 95, body, misc=0), "not a cube map")
    bad("legacy_no_cube_flag", dds_file(2, 1, None, bytes(6 * 2 * 2 * 8), fourcc=113), "not a cube map")
    bad("width_is_not_height", dds_file(8, 4, 95, body, height=4), "not a cube map")
    bad("width0", dds_file(0, 1, 95, body), "cube map size out of range (1..8192)")
    bad("width8193", dds_file(8193, 1, 95, body), "cube map size out of range (1..8192)")
    bad("width_2_to_the_31", dds_file(1 << 31, 1, 95, body), "cube map size out of range (1..8192)")
    bad("mips15", dds_file(8192, 15, 95, body), "mip count 15 exceeds the full chain of a 8192 cube")
    bad("mips_one_beyond", dds_file(8, 5, 95, body + bytes(6 * 16)), "mip count 5 exceeds the full chain of a 8 cube")
    bad("mips_one_beyond_5", dds_file(5, 4, 10, bytes(6 * 8 * (25 + 4 + 1 + 1))), "mip count 4 exceeds the full chain of a 5 cube")
    bad("mips_all_ones", dds_file(8, 0xFFFFFFFF, 95, body), "mip count 4294967295 exceeds the full chain of a 8 cube")
    for dxgi in (0, 94, 97, 98, 0x7FFFFFFF, 0xFFFFFFFF):
        bad("dxgi_%x" % dxgi, dds_file(8, 4, dxgi, body), "unsupported DXGI format %d" % (dxgi if dxgi < 1 << 31 else dxgi - (1 << 32)))
    return files


def test_dds_loader_program_plain_and_sanitized(built, tmp_path):
    files = loader_files()
    assert len(set(n for n, _, _ in files)) == len(files)
    paths = []
    for name, data, _ in files:
        p = tmp_path / (name + ".dds")
        p.write_bytes(data)
        paths.append(str(p))
    want = "".join("%s.dds: %s\n" % (name, line) for name, _, line in files)
    outputs = []
    for sanitize in (False, True):
        exe = compile_main(str(tmp_path / ("dds_loader_main" + ("_san" if sanitize else ""))), sanitize)
        r = subprocess.run([exe] + paths + [str(tmp_path / "missing.dds")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        outputs.append(r.stdout)
    assert outputs[0] == outputs[1]
    missing = "missing.dds: error: cannot open %s\n" % (tmp_path / "missing.dds")
    assert outputs[0] == want + missing, "\n".join(a + "   <->   " + b for a, b in zip(outputs[0].splitlines(), (want + missing).splitlines()) if a != b)
    # where the oracle's reader takes a file too, it finds the same cube
    o = O.Oracle(8, 8, threads=1)
    try:
        taken = 0
        for (name, _, line), p in zip(files, paths):
            if line.startswith("error"):
                continue
            try:
                o.set_env_dds(p)
            except IOError:
                assert name.startswith("legacy") or name == "cube_by_caps2_only", name          # the oracle reads DX10 cubes only
                continue
            size, mips, tex = o.env_texels()
            assert "size %d mips %d " % (size, mips) in line and tex.shape[0] == 6 * sum(max(size >> m, 1) ** 2 for m in range(mips)), (name, size, mips)
            taken += 1
        assert taken >= 30
    finally:
        o.close()
