"""Environments from images on the GPU (rtggx_set_env_image, rtggx_generate_env_mips; env.hip envCrossKernel, envEquirectKernel,
envMipKernel): RTGGX_BUF_ENV against the restatement tests/envimage_ref.py -- bit for bit for crosses and for the chain, within a derived
bound of the float64 model for panoramas --, the tail shared with rtggx_set_env (frames, SH, still-sky runs), the refusals, and the
executable's flags."""
import os
import subprocess

import numpy as np
import pytest

import assets
import env_cases as EC
import envimage_ref as E
import gpu_support as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "raytracedggx_amd", "RayTracedGGX")


@pytest.fixture(scope="module")
def ctx(built):
    from raytracedggx_amd import capi
    c = capi.Context(32, 32)
    yield c
    c.close()


def assert_same_texels(got, want, what):
    assert got.shape == want.shape, "%s: %s texels, restated %s" % (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d texels differ, first: texel %d = %s, restated %s" % (
        what, bad.size, got.shape[0], bad[0], ["%04x" % v for v in got[bad[0]]], ["%04x" % v for v in want[bad[0]]])


def random_floats(rng, H, W):
    """Ordinary radiance with, at random, zeros of both signs, negatives, NaN, infinities, values above the largest half and far above it;
    no fp32 denormal."""
    f = rng.uniform(0.0, 8.0, (H, W, 3)).astype(np.float32)
    kind = rng.integers(0, 16, (H, W, 3))
    f[kind == 0] = 0.0
    f[kind == 1] = -0.0
    f[kind == 2] = -rng.uniform(0.0, 8.0, int((kind == 2).sum())).astype(np.float32)
    f[kind == 3] = np.nan
    f[kind == 4] = np.inf
    f[kind == 5] = -np.inf
    f[kind == 6] = rng.uniform(65504.0, 66000.0, int((kind == 6).sum())).astype(np.float32)
    f[kind == 7] = 3.0e38
    f[kind == 8] = rng.uniform(2000.0, 65504.0, int((kind == 8).sum())).astype(np.float32)
    f[kind == 9] = 2.0 ** rng.integers(-100, -10, int((kind == 9).sum())).astype(np.float32)
    return f


# ---- 1. crosses --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [1, 2, 3, 5, 6, 13, 16, 33])
@pytest.mark.parametrize("pixels", [E.RGBE8, E.RGB32F], ids=["rgbe8", "rgb32f"])
@pytest.mark.parametrize("layout", [E.VCROSS, E.HCROSS], ids=["vcross", "hcross"])
def test_cross_equals_the_restatement_bit_for_bit(ctx, layout, pixels, cell):
    """Every level of RTGGX_BUF_ENV.  Cells 1 .. 33: chains with odd sides (13 -> 6 -> 3 -> 1, 33 -> 16, 5 -> 2, 3 -> 1) and even ones, 6 x 33^2
    texels are more than one workgroup.  RGBE exponents from 20 up (no fp32 denormal anywhere) to 160 (far above the largest half)."""
    from raytracedggx_amd import capi
    rng = np.random.default_rng(1000 * cell + 10 * layout + pixels)
    rows, cols = E.CELLS[layout]
    H, W = rows * cell, cols * cell
    image = E.random_rgbe(rng, H, W, 20, 160) if pixels == E.RGBE8 else random_floats(rng, H, W)
    ctx.set_env_image(layout, pixels, W, H, image)
    rgb = E.decode(pixels, image)
    want = E.pack(E.chain(E.cross_level0(layout, rgb)))
    got = ctx.readback(capi.BUF_ENV)
    assert_same_texels(got, want, "cell %d" % cell)
    assert ctx.buffer_size(capi.BUF_ENV) == 8 * 6 * sum(s * s for s in E.chain_sides(cell))
    if cell == 33 and pixels == E.RGB32F:      # what the input was meant to hold did reach the cube
        assert (got[:6 * cell * cell, :3] == 0x7BFF).any() and (got[:6 * cell * cell, :3] == 0).any() and not ((got & 0x7C00) == 0x7C00).any()


# ---- 2. rtggx_generate_env_mips ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cube", EC.all_cubes(), ids=lambda c: c.name)
def test_generated_chain_equals_the_restatement_and_keeps_level_0(ctx, cube):
    """rtggx_set_env with ONE level (level 0 of the env_cases cube: signed values, half denormals and +-65504 among them), then the chain:
    level 0 stays what it is, every level below is the restated chain of its halves widened to fp32."""
    from raytracedggx_amd import capi
    level0 = cube.codes[0]
    ctx.set_env(capi.FORMAT_RGBA16F, cube.size, 1, level0.reshape(-1))
    np.testing.assert_array_equal(ctx.readback(capi.BUF_ENV), level0.reshape(-1, 4))
    ctx.generate_env_mips()
    levels = E.chain(level0[..., :3].copy().view(np.float16).astype(np.float32))
    want = np.concatenate([level0.reshape(-1, 4), E.pack(levels[1:])]) if len(levels) > 1 else level0.reshape(-1, 4)
    assert_same_texels(ctx.readback(capi.BUF_ENV), want, cube.name)
    # once more: the chain is rebuilt from the same level 0, and a cube that came with (other) levels below it loses them
    ctx.generate_env_mips()
    assert_same_texels(ctx.readback(capi.BUF_ENV), want, cube.name + ", again")
    if cube.mips > 1:
        ctx.set_env(capi.FORMAT_RGBA16F, cube.size, cube.mips, cube.dds_order())
        ctx.generate_env_mips()
        assert_same_texels(ctx.readback(capi.BUF_ENV), want, cube.name + ", over its own levels")


def test_generate_env_mips_needs_an_environment(built):
    from raytracedggx_amd import capi
    c = capi.Context(32, 32)
    try:
        with pytest.raises(capi.RtggxError, match="no environment"):
            c.generate_env_mips()
    finally:
        c.close()


# ---- 3. panoramas --------------------------------------------------------------------------------------------------------------------------
def panorama(rng, pixels, H, W):
    """Values that are 0 or lie in [2^-6, 64).  Why the range is kept moderate: a tap's coordinates are fp64 on the device and in the model,
    each off by a few 2^-53 relative (atan2 and asin of two libraries), which moves a tap by at most W x 2^-50 pixels and a value by that
    times the largest difference of two neighbours: 100 x 2^-50 x 64 = 5.7e-12.  That is below the bound's first term, 2^-23 |value|, for
    every value from 2^-14 up (7.3e-12), and below 2^-14 the half rounding is 2^-25 whatever the value.  Zeros, negatives and NaN (both 0
    once decoded) are among the float pixels, black pixels and zero mantissas among the RGBE ones."""
    if pixels == E.RGBE8:
        return E.random_rgbe(rng, H, W, 130, 134)
    f = rng.uniform(2.0 ** -6, 64.0, (H, W, 3)).astype(np.float32)
    kind = rng.integers(0, 12, (H, W, 3))
    f[kind == 0] = 0.0
    f[kind == 1] = -rng.uniform(0.0, 8.0, int((kind == 1).sum())).astype(np.float32)
    f[kind == 2] = np.nan
    return f


@pytest.mark.parametrize("size", [1, 4, 16, 32])
@pytest.mark.parametrize("source", [(2, 1), (8, 4), (9, 5), (64, 32), (100, 50)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pixels", [E.RGBE8, E.RGB32F], ids=["rgbe8", "rgb32f"])
def test_panorama_lies_within_the_derived_bound_of_the_float64_model(ctx, pixels, source, size):
    """Level 0, unpacked from its halves: the model's value +- (2^-23 |value| + the half rounding of the value) -- coordinates and weights are
    fp64 on the device, so what is left is one rounding to fp32 (2^-24) and the different last bits of two fp64 evaluations, then the
    rounding to a half.  Levels >= 1 against the restated fp32 chain run on the model's level 0: the two level 0 differ by one fp32 rounding
    per texel at most (2^-23), the chain's weights are positive and sum to 1, and its own roundings act on inputs that close: 2^-22 of the
    weighted mean of |parents| -- the level's own value, nothing here being negative -- plus the half rounding."""
    from raytracedggx_amd import capi
    W, H = source
    rng = np.random.default_rng(100 * W + 10 * size + pixels)
    image = panorama(rng, pixels, H, W)
    ctx.set_env_image(E.EQUIRECT, pixels, W, H, image, cube_size=size)
    got = E.unpack(ctx.readback(capi.BUF_ENV), size)
    model0 = E.equirect_level0(E.decode(pixels, image), size)
    ref = E.chain(model0.astype(np.float32))
    assert len(got) == len(ref) == len(E.chain_sides(size))
    for m, (g, r) in enumerate(zip(got, ref)):
        value = model0 if m == 0 else r.astype(np.float64)
        tol = (2.0 ** -23 if m == 0 else 2.0 ** -22) * np.abs(value) + E.half_rounding(value)
        err = np.abs(g - value)
        print("%dx%d -> %d, level %d: largest |gpu - model| / bound = %.4f" % (W, H, size, m, (err / tol).max()))
        assert (err <= tol).all(), "%dx%d -> %d, level %d: texel %d is %.4f bounds from the model (%r vs %r)" % (
            W, H, size, m, (err / tol).argmax(), (err / tol).max(), g.reshape(-1)[(err / tol).argmax()], value.reshape(-1)[(err / tol).argmax()])
    assert model0.max() > 0.0


def test_panorama_default_cube_size(ctx):
    """cube_size 0: the largest power of two <= width / 4."""
    from raytracedggx_amd import capi
    rng = np.random.default_rng(8)
    for W, H in ((100, 50), (64, 32), (2, 1), (35, 9)):
        ctx.set_env_image(E.EQUIRECT, E.RGB32F, W, H, panorama(rng, E.RGB32F, H, W))
        size = E.default_cube_size(W)
        assert ctx.buffer_size(capi.BUF_ENV) == 8 * 6 * sum(s * s for s in E.chain_sides(size)), (W, size)


# ---- 4. the same tail as rtggx_set_env ---------------------------------------------------------------------------------------------------
def dds_order(buf, size):
    """RTGGX_BUF_ENV (mip-major, uint16 [texels, 4]) of a full chain -> the order rtggx_set_env takes (per face its chain)."""
    sides, at, levels = E.chain_sides(size), 0, []
    for s in sides:
        levels.append(buf[at:at + 6 * s * s].reshape(6, s * s * 4)); at += 6 * s * s
    return np.concatenate([levels[m][f] for f in range(6) for m in range(len(sides))]), len(sides)


ALL = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS


def smooth_cross(cell):
    def f(d):
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        return np.stack([1.5 + d[:, 0] + 0.3 * d[:, 1] * d[:, 2], 2.0 + np.sin(2.0 * d[:, 1]) + d[:, 2], 1.0 + d[:, 0] * d[:, 1] + 0.5 * d[:, 2]], axis=1)
    return E.paint_cross(E.VCROSS, cell, f).astype(np.float32)


def test_image_environment_renders_like_the_same_cube_through_set_env(built):
    """Three 100 x 54 bunny frames after rtggx_set_env_image; a twin context given rtggx_set_env(RGBA16F, the read-back of RTGGX_BUF_ENV)
    produces every buffer through the back buffer bit-identically.  The SH coefficients are held to what two projections of ONE cube are held
    to (tests/test_gpu_env.py): the projection adds its workgroups' sums with fp64 atomics, whose order moves the last bits -- measured here:
    -1.7e-16 against -1.5e-16 where the exact coefficient is 0 --, so both contexts' coefficients lie within 2^-23 of the sum of magnitudes
    of the float64 model's, and of each other.  Then, in mid-run on a still camera with sky tiles left alone, another image: the runs end
    (rtggx_debug_sky_runs reads 0) and the twin follows again."""
    import env_ref as R
    from raytracedggx_amd import capi
    W, H, cell = 100, 54, 13
    a, b = G.app(W, H), G.app(W, H)
    try:
        def give(image, layout, width, height, size, **kw):
            a.context.set_env_image(layout, E.RGB32F, width, height, image, **kw)
            env = a.context.readback(capi.BUF_ENV)
            data, mips = dds_order(env, size)
            b.context.set_env(capi.FORMAT_RGBA16F, size, mips, data)
            np.testing.assert_array_equal(b.context.readback(capi.BUF_ENV), env)
            return R.sh_project(E.unpack(env, size)[0], size)

        def same_sh(model, label):
            want, mag = model
            sa, sb = (x.context.readback(capi.BUF_SH_COEFFS).astype(np.float64).reshape(9, 3) for x in (a, b))
            assert (np.abs(sa - want) <= EC.SH_BOUND * mag).all() and (np.abs(sb - want) <= EC.SH_BOUND * mag).all(), label
            assert (np.abs(sa - sb) <= EC.SH_BOUND * mag).all() and np.abs(sa).max() > 0.1, label

        model = give(smooth_cross(cell), E.VCROSS, 3 * cell, 4 * cell, cell)
        for f in range(3):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, ALL), G.images(b, ALL), "frame %d" % f)
            same_sh(model, "SH, frame %d" % f)
        assert G.images(a, ("back",))["back"].any()
        for f in range(12):      # three times round the input sets: sky tiles are left alone
            G.frame(a); G.frame(b)
        runs, threshold = a.context.sky_runs()
        assert (runs >= threshold).sum() > 0
        rng = np.random.default_rng(4)
        model = give(panorama(rng, E.RGB32F, 20, 40), E.EQUIRECT, 40, 20, 6, cube_size=6)
        runs, _ = a.context.sky_runs()
        assert runs.max() == 0
        for f in range(3):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, ALL), G.images(b, ALL), "after the second image, frame %d" % f)
            same_sh(model, "SH after the second image, frame %d" % f)
    finally:
        a.OnDestroy(); b.OnDestroy()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_environment_and_the_frame_as_they_were(built):
    from raytracedggx_amd import capi
    W, H = 100, 54
    a, b = G.app(W, H), G.app(W, H)
    try:
        for f in range(12):
            G.frame(a); G.frame(b)
        env = a.context.readback(capi.BUF_ENV)
        runs = a.context.sky_runs()[0]
        assert runs.max() > 0
        c = a.context
        f32, rgbe = np.ones((12, 9, 3), np.float32), np.full((12, 9, 4), 128, np.uint8)
        for args, kw, word in (
                ((E.VCROSS, E.RGB32F, 9, 12, None), {}, "null data"),
                ((E.VCROSS, E.RGB32F, 9, 12, f32.reshape(-1)[:-1]), {}, "bytes given"),
                ((E.VCROSS, E.RGBE8, 9, 12, rgbe.reshape(-1)[:-1]), {}, "bytes given"),
                ((E.EQUIRECT, E.RGB32F, 0, 12, f32), {}, "0 x 12"), ((E.EQUIRECT, E.RGB32F, 9, 0, f32), {}, "9 x 0"),
                ((E.EQUIRECT, E.RGB32F, 16385, 1, f32), {}, "more than 16384 x 8192"), ((E.EQUIRECT, E.RGBE8, 1, 8193, rgbe), {}, "more than 16384 x 8192"),
                ((E.VCROSS, E.RGB32F, 12, 9, f32), {}, "no vertical cross"), ((E.HCROSS, E.RGB32F, 9, 12, f32), {}, "no horizontal cross"),
                ((E.VCROSS, E.RGB32F, 9, 11, f32), {}, "no vertical cross"), ((E.HCROSS, E.RGBE8, 8, 3, rgbe), {}, "no horizontal cross"),
                ((E.VCROSS, E.RGB32F, 3 * 4097, 4 * 4097, f32), {}, "more than 4096"),
                ((3, E.RGB32F, 9, 12, f32), {}, "unknown layout"), ((-1, E.RGB32F, 9, 12, f32), {}, "unknown layout"),
                ((E.VCROSS, 2, 9, 12, f32), {}, "unknown pixel format"), ((E.VCROSS, -1, 9, 12, f32), {}, "unknown pixel format"),
                ((E.VCROSS, E.RGB32F, 9, 12, f32), {"cube_size": 3}, "never resampled"),
                ((E.EQUIRECT, E.RGB32F, 9, 12, f32), {"cube_size": 4097}, "more than 4096")):
            with pytest.raises(capi.RtggxError, match=word):
                c.set_env_image(*args, **kw)
            np.testing.assert_array_equal(c.readback(capi.BUF_ENV), env, err_msg=word)
        np.testing.assert_array_equal(a.context.sky_runs()[0], runs)      # not a run has ended
        for f in range(2):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, ALL), G.images(b, ALL), "after the refusals, frame %d" % f)
        # and what is accepted at the edges of those rules is: the same image with the sizes right
        c.set_env_image(E.VCROSS, E.RGB32F, 9, 12, f32)
        c.set_env_image(E.EQUIRECT, E.RGB32F, 9, 12, f32, cube_size=3)
        assert c.buffer_size(capi.BUF_ENV) == 8 * 6 * (9 + 1)
    finally:
        a.OnDestroy(); b.OnDestroy()


# ---- 6. the executable ---------------------------------------------------------------------------------------------------------------------
def one_level_dds(level0):
    """uint16 [6, s, s, 4] -> the bytes of a DX10 DDS cube of R16G16B16A16_FLOAT with one level."""
    s = level0.shape[1]
    head = np.zeros(37, np.uint32)      # "DDS ", the 124-byte header, the 20-byte DX10 header
    head[0] = 0x20534444
    head[1], head[2], head[3], head[4], head[7] = 124, 0x1007, s, s, 1
    head[19], head[20], head[21] = 32, 0x4, 0x30315844      # pixel format: size, DDPF_FOURCC, "DX10"
    head[27], head[28] = 0x1008, 0xFE00                      # caps: complex | texture; caps2: a cube map with all six faces
    head[32], head[33], head[34], head[35] = 10, 3, 0x4, 1   # DXGI_FORMAT_R16G16B16A16_FLOAT, TEXTURE2D, TEXTURECUBE, one cube
    return head.tobytes() + np.ascontiguousarray(level0, np.uint16).tobytes()


def test_executable_takes_image_environments_and_builds_a_missing_chain(built, tmp_path):
    from raytracedggx_amd import app, capi
    rng = np.random.default_rng(9)
    scene = ["-mesh", assets.path("bunny.obj"), "-width", "100", "-height", "54", "-frames", "2"]

    def write(name, data):
        with open(str(tmp_path / name), "wb") as f:
            f.write(data)
        return str(tmp_path / name)

    cross = E.random_rgbe(rng, 64, 48, 130, 138)
    pano = rng.uniform(0.0, 4.0, (32, 64, 3)).astype(np.float32)
    cube = EC.random_cube(12, 3)
    files = {"cross": write("cross.hdr", E.hdr_bytes(cross, rle=True)), "pano": write("pano.pfm", E.pfm_bytes(pano)), "dds": write("one.dds", one_level_dds(cube.codes[0]))}
    generated = np.concatenate([cube.codes[0].reshape(-1, 4), E.pack(E.chain(cube.codes[0][..., :3].copy().view(np.float16).astype(np.float32))[1:])])
    cases = (("cross", [], E.pack(E.chain(E.cross_level0(E.VCROSS, E.decode(E.RGBE8, cross))))),
             ("pano", ["-envsize", "8"], None),
             ("dds", ["-envmips"], generated),
             ("dds", [], cube.codes[0].reshape(-1, 4)))
    for name, extra, want in cases:
        dump = str(tmp_path / (name + "%d.ppm" % len(extra)))
        r = subprocess.run([EXE] + scene + ["-env", files[name], "-dump", dump] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "wrote " + dump in r.stdout, (name, r.stdout, r.stderr)
        body = open(dump, "rb").read()
        assert body.startswith(b"P6\n100 54\n255\n") and len(set(body[15:])) > 16, name      # a picture, not a flat colour
        # the same command line through the application object: what the environment became
        a = app.RayTracedGGX(scene + ["-env", files[name]] + extra)
        try:
            env = a.context.readback(capi.BUF_ENV)
            if want is not None:
                assert_same_texels(env, want, name + " " + " ".join(extra))
            else:
                got = E.unpack(env, 8)      # every level, by the bounds of the panorama test
                model0 = E.equirect_level0(E.decode(E.RGB32F, pano), 8)
                ref = E.chain(model0.astype(np.float32))
                assert len(got) == len(ref) == 4
                for m, (g, r) in enumerate(zip(got, ref)):
                    value = model0 if m == 0 else r.astype(np.float64)
                    assert (np.abs(g - value) <= (2.0 ** -23 if m == 0 else 2.0 ** -22) * np.abs(value) + E.half_rounding(value)).all(), m
        finally:
            a.OnDestroy()
