"""Environments from images without a GPU: the restatement tests/envimage_ref.py against what can be known without the kernels (the
float64 sampler of tests/env_ref.py, constants, a chain computed by hand), the Radiance / PFM readers of host/EnvImageLoader.h through
rtggx_host_load_env_image on files written here, the executable's refusals, and the readers under AddressSanitizer and UBSan in a
stand-alone program (tests/envimage_readers_main.cpp) run as a child process."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import assets
import env_ref as R
import envimage_ref as E
import host_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def smooth(d):
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.stack([1.5 + d[:, 0] + 0.3 * d[:, 1] * d[:, 2], 2.0 + np.sin(2.0 * d[:, 1]) + d[:, 2], 1.0 + d[:, 0] * d[:, 1] + 0.5 * d[:, 2]], axis=1)


# ---- 1. the cross tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [E.VCROSS, E.HCROSS], ids=["vcross", "hcross"])
def test_cross_tables_are_continuous_and_return_the_painted_function(layout):
    """A cross painted from a smooth function of direction has no step at any seam between two cells of the image (nor, for the vertical
    cross, from the bottom of -Z back to the top of +Y), and the cube extracted from it returns the function through the float64 sampler."""
    c = 32
    img = E.paint_cross(layout, c, smooth)
    cells = E.CROSS[layout]
    inner = max(np.abs(np.diff(img[c:2 * c, c:2 * c], axis=0)).max(), np.abs(np.diff(img[c:2 * c, c:2 * c], axis=1)).max())      # texel to texel inside +Z
    seams = 0
    for (r, col) in cells:
        if (r + 1, col) in cells:
            seams += 1
            assert np.abs(img[(r + 1) * c - 1, col * c:(col + 1) * c] - img[(r + 1) * c, col * c:(col + 1) * c]).max() <= 1.5 * inner, (r, col)
        if (r, col + 1) in cells:
            seams += 1
            assert np.abs(img[r * c:(r + 1) * c, (col + 1) * c - 1] - img[r * c:(r + 1) * c, (col + 1) * c]).max() <= 1.5 * inner, (r, col)
    assert seams == 5
    if layout == E.VCROSS:
        assert np.abs(img[4 * c - 1, c:2 * c] - img[0, c:2 * c]).max() <= 1.5 * inner
    d = np.random.default_rng(1).normal(size=(4000, 3))
    _, u, v = R.face_uv(d)
    err, err_all = {}, {}
    for side in (c, 2 * c):
        cube = E.cross_level0(layout, E.decode(E.RGB32F, E.paint_cross(layout, side, smooth).astype(np.float32)))
        lo, hi = R.environment([cube.astype(np.float64)], side, d, np.zeros(4000))
        e = np.maximum(np.abs(lo - smooth(d)), np.abs(hi - smooth(d))).max(axis=1)
        inside = (np.abs(u) < 1.0 - 1.0 / side) & (np.abs(v) < 1.0 - 1.0 / side)      # all four taps on the direction's own face
        err[side], err_all[side] = e[inside].max(), e.max()
    # Bilinear interpolation of a smooth function inside a face: second order in the texel size h = 2 / side -- h^2 / 8 times the second
    # derivatives along both axes (below 20 together), and a quarter at twice the side (a third allowed).  A tap across an edge reads the
    # neighbouring face's texel, whose centre lies up to h / 2 from where the weights assume it: half the weight x h / 2 x the gradient (< 4).
    assert err[c] < (2.0 / c) ** 2 / 8.0 * 20.0 and err[2 * c] < err[c] / 3.0, err
    assert err_all[c] < 0.5 * (1.0 / c) * 4.0 and err_all[2 * c] < 0.5 * (0.5 / c) * 4.0, err_all
    cube = E.cross_level0(layout, E.decode(E.RGB32F, img.astype(np.float32)))
    # and a wrong table is seen: the horizontal table on the vertical cross's -Z (no turn) turns a whole face
    wrong = cube.copy(); wrong[5] = wrong[5][::-1, ::-1]
    lo, _ = R.environment([wrong.astype(np.float64)], c, d, np.zeros(4000))
    assert np.abs(lo - smooth(d)).max() > 1.0


def test_decode_and_clamp():
    rgbe = np.array([[[128, 64, 1, 136], [255, 255, 255, 0], [0, 0, 0, 200], [255, 1, 128, 152], [128, 0, 0, 20], [1, 2, 3, 1]]], np.uint8)
    got = E.decode(E.RGBE8, rgbe)[0]
    np.testing.assert_array_equal(got[0], [128.0, 64.0, 1.0])
    np.testing.assert_array_equal(got[1], [0, 0, 0])
    np.testing.assert_array_equal(got[2], [0, 0, 0])
    np.testing.assert_array_equal(got[3], [65504.0, 65504.0, 65504.0])      # 255 x 65536, 65536, 128 x 65536: all above the largest half
    np.testing.assert_array_equal(got[4], np.array([2.0 ** -109, 0, 0], np.float32))
    np.testing.assert_array_equal(got[5].view(np.uint32), np.array([2.0 ** -135, 2.0 ** -134, 3 * 2.0 ** -135], np.float32).view(np.uint32))      # fp32 denormals, exact
    f = np.array([[[0.0, -0.0, -1.0], [np.nan, np.inf, -np.inf], [65504.0, 65505.0, 1e-30], [1e-45, 3.5, 7e4]]], np.float32)
    got = E.decode(E.RGB32F, f)[0]
    np.testing.assert_array_equal(got.view(np.uint32), np.array([[0, 0, 0], [0, 65504.0, 0], [65504.0, 65504.0, 1e-30], [1e-45, 3.5, 65504.0]], np.float32).view(np.uint32))


# ---- 2. the chain ----------------------------------------------------------------------------------------------------------------------
def test_chain_keeps_a_constant():
    """Exactly where every side down to 1 is even.  An odd axis (p = 2 q + 1) takes the integer weights q - i, q, i + 1, which sum to p: on a
    constant the result is within 2 x 2^-24 relative -- one spacing of fp32 -- of it, per application of the rule.  (Over a whole chain the
    applications add up: 13 -> 6 -> 3 -> 1 ends 2.9 x 2^-24 from the constant, 4095 5.9 x 2^-24; so the bound is asserted where it is true, per
    axis pass against the smallest and largest value the pass was given.)"""
    for size in (1, 2, 4, 16, 64):
        for v in (1.0, 0.1, 3.3, 65504.0, 2.0 ** -20):
            levels = E.chain(np.full((6, size, size, 3), v, np.float32))
            assert [l.shape[1] for l in levels] == E.chain_sides(size)
            for l in levels:
                assert (l == np.float32(v)).all()
    bound, odd_passes = 2.0 * 2.0 ** -24, 0
    for size in (3, 5, 6, 7, 13, 33, 77, 100, 255):
        for v in (1.0, 0.1, 3.3, 65504.0, 0.7, 1e-3, 2.9, 1.0 / 3.0):
            a = np.full((6 if size < 100 else 1, size, size, 3), v, np.float32)
            sides = [size]
            while a.shape[1] > 1:
                for axis in (2, 1):
                    odd = a.shape[axis] % 2 == 1
                    b = E._halve(a, axis)
                    lo, hi = float(a.min()), float(a.max())
                    if odd:
                        odd_passes += 1
                        assert lo * (1.0 - bound) <= float(b.min()) and float(b.max()) <= hi * (1.0 + bound), (size, v, a.shape)
                    else:
                        assert lo <= float(b.min()) and float(b.max()) <= hi and (lo != hi or (b == a.flat[0]).all()), (size, v, a.shape)
                    a = b
                sides.append(a.shape[1])
            assert sides == E.chain_sides(size) and sides[-1] == 1
            assert (E.chain(np.full((1, size, size, 3), v, np.float32))[-1] == a[:1]).all()      # (the passes above ARE the chain)
    assert odd_passes > 100


def test_chain_of_five_by_hand():
    """5 -> 2 -> 1 on small integers, where every fp32 operation but the division is exact.  One row (1 2 3 4 5) repeated: horizontally
    child 0 = (2 x 1 + 2 x 2 + 1 x 3) / 5 = 9 / 5, child 1 = (1 x 3 + 2 x 4 + 2 x 5) / 5 = 21 / 5; vertically the same weights on equal rows:
    (2 a + 2 a + a) / 5 with a = fl(9 / 5) -- 5 a is not a float, so it is spelled out."""
    f = np.float32
    row = np.array([1, 2, 3, 4, 5], np.float32)
    level = np.broadcast_to(row[None, None, :, None], (6, 5, 5, 3)).astype(np.float32)
    l1 = E.next_level(level)
    a, b = f(9) / f(5), f(21) / f(5)
    va = ((f(2) * a + f(2) * a) + f(1) * a) / f(5)
    va1 = ((f(1) * a + f(2) * a) + f(2) * a) / f(5)
    vb = ((f(2) * b + f(2) * b) + f(1) * b) / f(5)
    vb1 = ((f(1) * b + f(2) * b) + f(2) * b) / f(5)
    np.testing.assert_array_equal(l1[0, :, :, 0], np.array([[va, vb], [va1, vb1]], np.float32))
    l2 = E.next_level(l1)
    h0, h1 = (va + vb) / f(2), (va1 + vb1) / f(2)
    assert l2.shape == (6, 1, 1, 3) and l2[3, 0, 0, 2] == (h0 + h1) / f(2)
    assert abs(float(l2[0, 0, 0, 0]) - 3.0) < 1e-6
    # a column instead of a row: the vertical pass alone; child (0, .) = 9 / 5, child (1, .) = 21 / 5, the horizontal pass saw constants
    l1t = E.next_level(np.ascontiguousarray(level.transpose(0, 2, 1, 3)))
    ha = ((f(2) * f(1) + f(2) * f(1)) + f(1) * f(1)) / f(5)      # = 1 exactly: a constant row stays
    assert ha == f(1)
    np.testing.assert_array_equal(l1t[0, :, 0, 0], np.array([a, b], np.float32))
    # an asymmetric face: the order "horizontal first" matters in the last bit, so check one texel of a random face against scalars
    rng = np.random.default_rng(4)
    t = rng.uniform(0, 8, (6, 5, 5, 3)).astype(np.float32)
    got = E.next_level(t)[2, 1, 0, 1]
    hx = [((f(2) * t[2, y, 0, 1] + f(2) * t[2, y, 1, 1]) + f(1) * t[2, y, 2, 1]) / f(5) for y in (2, 3, 4)]
    assert got == ((f(1) * hx[0] + f(2) * hx[1]) + f(2) * hx[2]) / f(5)
    # the packed layout: mip-major, six faces per mip
    buf = E.pack(E.chain(t))
    assert buf.shape == (6 * (25 + 4 + 1), 4) and (buf[:, 3] == 0x3C00).all()
    np.testing.assert_array_equal(E.unpack(buf, 5)[1], E.next_level(t).astype(np.float16).astype(np.float64))


def test_panorama_model_directions():
    """+Z in the middle of the image, +X to its right, +Y in the top row: a panorama painted from a smooth function of direction comes back
    through the model and the sampler."""
    W, H, size = 256, 128, 32
    lon = ((np.arange(W) + 0.5) / W - 0.5) * 2.0 * np.pi
    lat = (0.5 - (np.arange(H) + 0.5) / H) * np.pi
    d = np.stack([np.cos(lat)[:, None] * np.sin(lon)[None, :], np.repeat(np.sin(lat)[:, None], W, axis=1), np.cos(lat)[:, None] * np.cos(lon)[None, :]], axis=2)
    img = smooth(d.reshape(-1, 3)).reshape(H, W, 3)
    cube = E.equirect_level0(img, size)
    c, _, _, _ = R.texel_centre_dirs(size)
    assert np.abs(cube.reshape(-1, 3) - smooth(c)).max() < 2e-3      # bilinear over pixels of 2 pi / 256
    assert E.default_cube_size(2048) == 512 and E.default_cube_size(100) == 16 and E.default_cube_size(2) == 1 and E.default_cube_size(8) == 2


# ---- 3. the readers --------------------------------------------------------------------------------------------------------------------
def write(path, data):
    with open(str(path), "wb") as f:
        f.write(data)
    return str(path)


def test_readers_round_trip(built, tmp_path):
    from raytracedggx_amd import app, capi
    assert "rtggx_host_load_env_image" in app.HOST_EXPORTS
    rng = np.random.default_rng(2)
    for k, (H, W) in enumerate(((4, 3), (1, 1), (6, 8), (64, 48), (32, 64), (5, 130), (3, 7))):
        p = E.random_rgbe(rng, H, W)
        p[0, :min(W, 5)] = p[0, 0]      # runs for the run-length writer, and ...
        if W >= 8:
            p[-1, :, 1] = 9             # ... one longer than 127 where the row is
        for rle in ((False, True) if W >= 8 else (False,)):
            for magic in (b"#?RADIANCE", b"#?RGBE"):
                path = write(tmp_path / ("i%d_%d.bin" % (k, rle)), E.hdr_bytes(p, rle=rle, magic=magic))      # (the name tells nothing: the first bytes do)
                px, layout, img = app.load_env_image(path)
                assert px == capi.PIXELS_RGBE8 and img.shape == (H, W, 4)
                np.testing.assert_array_equal(img, p)
                assert layout == {(4, 3): capi.ENV_VCROSS, (64, 48): capi.ENV_VCROSS, (6, 8): capi.ENV_HCROSS, (32, 64): capi.ENV_EQUIRECT}.get((H, W), -1)
        f = rng.uniform(-4, 4, (H, W, 3)).astype(np.float32)
        f[0, 0] = (np.nan, np.inf, -0.0)
        path = write(tmp_path / ("f%d.dat" % k), E.pfm_bytes(f))
        px, layout, img = app.load_env_image(path)
        assert px == capi.PIXELS_RGB32F and img.shape == (H, W, 3)
        np.testing.assert_array_equal(img.view(np.uint32), f.view(np.uint32))
    # CR LF header lines and a scale other than -1 (its magnitude is not applied)
    path = write(tmp_path / "crlf.hdr", E.hdr_bytes(p, rle=False).replace(b"\n\n", b"\r\n\r\n", 1))
    np.testing.assert_array_equal(app.load_env_image(path)[2], p)
    path = write(tmp_path / "scale.pfm", E.pfm_bytes(f, scale=b"-2.5"))
    np.testing.assert_array_equal(app.load_env_image(path)[2].view(np.uint32), f.view(np.uint32))


def test_readers_refuse_what_they_cannot_read(built, tmp_path):
    from raytracedggx_amd import app
    rng = np.random.default_rng(3)
    p = E.random_rgbe(rng, 6, 16)
    p[2, 3:9] = p[2, 3]
    good, good_rle = E.hdr_bytes(p), E.hdr_bytes(p, rle=True)
    f = rng.uniform(0, 4, (6, 8, 3)).astype(np.float32)
    pfm = E.pfm_bytes(f)
    old = p.copy(); old[1, 5] = (1, 1, 1, 4)
    body = good_rle.index(b"-Y 6 +X 16\n") + len(b"-Y 6 +X 16\n")
    over = bytearray(good_rle); over[body + 4] = 128 + 17; over[body + 5:body + 5] = b"\x07"      # a run of 17 in a scanline of 16
    zero = bytearray(good_rle); zero[body + 4] = 0
    width = bytearray(good_rle); width[body + 3] = 15
    cases = [
        (b"", "neither"), (b"DDS rubbish", "neither"), (b"P6\n2 2\n255\n" + bytes(12), "neither"),
        (b"#?RADIANC\n\n", "not a Radiance file"), (good[:8], "not a Radiance file"), (good[:30], "truncated Radiance header"),
        (E.hdr_bytes(p, fmt=b""), "without FORMAT"), (E.hdr_bytes(p, fmt=b"FORMAT=32-bit_rle_xyze"), "unsupported Radiance format"),
        (E.hdr_bytes(p, resolution=b"+Y 6 +X 16"), "only \"-Y H +X W\""), (E.hdr_bytes(p, resolution=b"-Y 6 -X 16"), "only \"-Y H +X W\""),
        (E.hdr_bytes(p, resolution=b"+X 16 -Y 6"), "only \"-Y H +X W\""), (E.hdr_bytes(p, resolution=b"-Y 6 +X 16 x"), "only \"-Y H +X W\""),
        (E.hdr_bytes(p, resolution=b"-Y 0 +X 16"), "1 .. 16384"), (E.hdr_bytes(p, resolution=b"-Y 6 +X 20000"), "1 .. 16384"),
        (good[:-1], "truncated Radiance file"), (good[:body + 10], "truncated Radiance file"), (good_rle[:-1], "truncated Radiance file"),
        (E.hdr_bytes(old), "old-style"), (bytes(over), "passes its end"), (bytes(zero), "length 0"), (bytes(width), "another width"),
        (b"PF", "not a colour PFM"), (b"Pf\n8 6\n-1.0\n" + bytes(576), "neither"), (b"PF\n8\n", "width and height"), (b"PF\n8 x\n-1\n", "width and height"),
        (b"PF\n8 -6\n-1.0\n" + bytes(576), "width and height"), (b"PF\n8 6\n", "scale"), (b"PF\n8 6\nabc\n" + bytes(576), "scale"),
        (E.pfm_bytes(f, scale=b"1.0"), "big-endian"), (E.pfm_bytes(f, scale=b"0"), "big-endian"), (pfm[:-1], "truncated PFM"), (pfm[:12], "truncated PFM"),
        (b"PF\n0 6\n-1.0\n", "1 .. 16384"), (b"PF\n99999 6\n-1.0\n", "1 .. 16384"),
    ]
    for k, (data, word) in enumerate(cases):
        with pytest.raises(IOError, match=re.escape(word)):
            app.load_env_image(write(tmp_path / ("bad%d" % k), data))
    with pytest.raises(IOError, match="cannot open"):
        app.load_env_image(str(tmp_path / "missing.hdr"))
    app.load_env_image(write(tmp_path / "good.hdr", good_rle))      # (the corrupted files above differ from a good one by what is named)


# ---- 4. the executable -----------------------------------------------------------------------------------------------------------------
def test_executable_refuses_envsize_with_a_cross_and_bad_flags(built, tmp_path):
    """Before anything touches a GPU: -envsize with a cross -- by the image's aspect ratio or by -envlayout --, unknown layouts, sizes out
    of range, an image whose aspect ratio tells no layout, a file that is neither a cube nor an image."""
    rng = np.random.default_rng(5)
    vcross = write(tmp_path / "v.hdr", E.hdr_bytes(E.random_rgbe(rng, 8, 6)))
    hcross = write(tmp_path / "h.pfm", E.pfm_bytes(rng.uniform(0, 2, (6, 8, 3))))
    odd = write(tmp_path / "odd.hdr", E.hdr_bytes(E.random_rgbe(rng, 5, 7)))
    bad = write(tmp_path / "bad.hdr", E.hdr_bytes(E.random_rgbe(rng, 8, 6))[:-3])
    junk = write(tmp_path / "junk.dds", b"nothing")
    scene = ("-mesh", assets.path("triangle.obj"), "-width", "64", "-height", "64")
    host_support.executable_refuses([
        (["-env", vcross, "-envsize", "8"], "a cross is never resampled"), (["-env", hcross, "-envsize", "8"], "a cross is never resampled"),
        (["-env", odd, "-envlayout", "vcross", "-envsize", "8"], "a cross is never resampled"),
        (["-env", assets.path("rnl_cross.dds"), "-envlayout", "hcross", "-envsize", "4"], "a cross is never resampled"),
        (["-env", assets.path("rnl_cross.dds"), "-envlayout", "cube"], "-envlayout: equirect, vcross or hcross"),
        (["-env", assets.path("rnl_cross.dds"), "-envlayout"], "-envlayout: equirect, vcross or hcross"),
        (["-env", assets.path("rnl_cross.dds"), "-envsize", "0"], "-envsize: the side of the cube, 1 to 4096"),
        (["-env", assets.path("rnl_cross.dds"), "-envsize", "4097"], "-envsize: the side of the cube, 1 to 4096"),
        (["-env", odd], "name the layout with -envlayout"), (["-env", bad], "truncated Radiance file"), (["-env", junk], "not a DDS file"),
        (["-env", str(tmp_path / "missing.hdr")], "cannot open"),
    ], scene=scene)


def test_c_abi_and_host_declare_the_new_entry_points(built):
    host_support.declared_exported_bound("rtggx_set_env_image", r"int\s+rtggx_set_env_image\(rtggx_context\* ctx, int layout, int pixels, uint32_t width, uint32_t height, const void\* data, size_t bytes,\s+uint32_t cube_size\);",
                                         defines=(r"RTGGX_ENV_EQUIRECT = 0, RTGGX_ENV_VCROSS = 1, RTGGX_ENV_HCROSS = 2", r"RTGGX_PIXELS_RGBE8 = 0, RTGGX_PIXELS_RGB32F = 1"))
    host_support.declared_exported_bound("rtggx_generate_env_mips", r"int\s+rtggx_generate_env_mips\(rtggx_context\* ctx\);")
    from raytracedggx_amd import capi
    assert (capi.ENV_EQUIRECT, capi.ENV_VCROSS, capi.ENV_HCROSS, capi.PIXELS_RGBE8, capi.PIXELS_RGB32F) == (0, 1, 2, 0, 1)
    assert (E.EQUIRECT, E.VCROSS, E.HCROSS, E.RGBE8, E.RGB32F) == (0, 1, 2, 0, 1)


# ---- 5. the readers under the sanitizers -------------------------------------------------------------------------------------------------
def test_readers_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/envimage_readers_main.cpp, a program of its own: the readers over a valid run-length .hdr, a flat one and a .pfm, over every
    truncation of each, byte by byte, and over each file with every byte in turn replaced by nine values (0, 1, 2, 127 .. 130, 200, 255: run
    lengths that are empty, literal, the longest, the shortest run, too long).  It must end clean: an error string for every bad file, and
    not a word from either sanitizer.  The runtimes are linked into the program (-static-libasan): nothing is preloaded and nothing
    is loaded into Python."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to build the stand-alone reader program with")
    exe = str(tmp_path / "envimage_readers")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                        os.path.join(ROOT, "tests", "envimage_readers_main.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b|unrecognized (command[- ]line )?option .*-fsanitize", r.stderr):
        pytest.skip("the sanitizer runtime is missing: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(6)
    p = E.random_rgbe(rng, 6, 16)
    p[1, 2:12] = p[1, 2]; p[4, :, 3] = 130
    files = {"rle.hdr": E.hdr_bytes(p, rle=True), "flat.hdr": E.hdr_bytes(p[:3, :5]), "image.pfm": E.pfm_bytes(rng.uniform(-1, 3, (3, 4, 3)))}
    for name, data in files.items():
        r = subprocess.run([exe, write(tmp_path / name, data)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (name, r.stdout, r.stderr)
        assert "truncations refused %d" % len(data) in r.stdout and re.search(r"corruptions parsed \d+ refused [1-9]", r.stdout), (name, r.stdout)
