"""The environment path on the GPU -- the cube-map sampler the frame kernels call (raytrace.hip environment(), environmentLevel0(), through
rtggx_debug_environment), the SH projection (env.hip shProjectKernel) and the uploads (decodeEnv) -- on the small synthetic cubes of
tests/env_cases.py, against the CPU oracle bit for bit AND against the float64 models of tests/env_ref.py, which are written from the
definitions and checked against the oracle and against known answers in tests/test_env_ref_host.py.

The frame tests compare whole images on one 256 x 256 cube; at that size every coordinate of the sampler is exact in fp32, and the oracle's
sampler is the kernel's text once more.  Here the sides are 1 ... 16, mostly no powers of two, the directions sit on the cube's edges and
corners, and the third opinion is independent.  The bounds are stated in env_cases.py (B, counted from the fp32 roundings; 2^-23 of the
sum of magnitudes for SH).  profiles/r09_env_mutations.txt tries seven mutations on these test functions with a mutated ORACLE in the
device's place (a host proxy for the model-based assertions; runs of mutated libraries on the device are not recorded there)."""
import numpy as np
import pytest

import env_cases as EC
import env_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CUBES = EC.all_cubes()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what, dirs, levels=None):
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    if bad.size:
        i = bad[0]
        raise AssertionError("%s: %d of %d directions differ, first: direction %d = %r level %r: %r vs %r" % (
            what, bad.size, got.shape[0], i, dirs[i].tolist(), None if levels is None else float(np.broadcast_to(levels, (dirs.shape[0],))[i]),
            got[i].tolist(), want[i].tolist()))


def outside(got, lo, hi, B):
    """Distance of got from [lo, hi] in units of B (0 inside), per direction."""
    B = np.asarray(B, np.float64).reshape(-1, 1)
    got = got.astype(np.float64)
    return (np.maximum(np.maximum(lo - got, got - hi), 0.0) / B).max(axis=1)


@pytest.fixture(scope="module")
def ctx(built):
    from raytracedggx_amd import capi
    c = capi.Context(32, 32)
    yield c
    c.close()


@pytest.mark.parametrize("cube", CUBES, ids=lambda c: c.name)
def test_sampler_equals_the_oracle_and_lies_in_the_model_interval(ctx, cube):
    from raytracedggx_amd import capi
    D, lv = EC.directions(cube.size), EC.levels_for(cube.mips)
    ctx.set_env(capi.FORMAT_RGBA16F, cube.size, cube.mips, cube.dds_order())
    np.testing.assert_array_equal(ctx.readback(capi.BUF_ENV), cube.mip_major())
    o = O.Oracle(8, 8, threads=1)
    try:
        o.set_env_rgba16f(cube.size, cube.mips, cube.mip_major())
        # one level per direction: integers, fractions, below 0, above the chain, one ulp either side of an integer
        got = ctx.debug_environment(D.d, lv)
        lo, hi = R.environment(cube.levels, cube.size, D.d, lv)
        far = outside(got, lo, hi, EC.bound(cube, lv))
        point = (lo == hi).all(axis=1)
        near = (np.abs(got - lo) / EC.bound(cube, lv)[:, None]).max(axis=1)[point].max() if point.any() else 0.0
        print("%s: GPU outside the model's interval by at most %.3f B; where the interval is a point, |gpu - model| <= %.3f B" % (cube.name, far.max(), near))
        assert_same_bits(got, EC.oracle_environment(o, D.d, lv), cube.name + ": GPU vs oracle", D.d, lv)
        assert far.max() <= 1.0, "%s: direction %d = %r level %r is %.3f B outside the model's interval" % (
            cube.name, far.argmax(), D.d[far.argmax()].tolist(), float(lv[far.argmax()]), far.max())
        # every integer level by itself
        for m in range(cube.mips):
            g = ctx.debug_environment(D.d, float(m))
            assert_same_bits(g, EC.oracle_environment(o, D.d, float(m)), "%s level %d: GPU vs oracle" % (cube.name, m), D.d, float(m))
            lo, hi = R.environment(cube.levels, cube.size, D.d, float(m))
            far = outside(g, lo, hi, EC.bound(cube, float(m)))
            assert far.max() <= 1.0, "%s level %d: direction %d is %.3f B outside the model's interval" % (cube.name, m, far.argmax(), far.max())
            if m == 0:
                g0 = g
        # the folded level-0 path of sky pixels and misses; it ignores the level
        assert_same_bits(ctx.debug_environment(D.d, lv, level0=True), g0, cube.name + ": environmentLevel0 vs environment(dir, 0)", D.d)
        assert_same_bits(ctx.debug_environment(D.d, -1.0), g0, cube.name + ": level -1 vs level 0", D.d)
        assert_same_bits(ctx.debug_environment(D.d, cube.mips + 0.5), ctx.debug_environment(D.d, float(cube.mips - 1)), cube.name + ": above the chain vs the last level", D.d)
        if cube.size & (cube.size - 1) == 0:
            # a power of two: every coordinate is exact, a direction through a texel's centre returns that texel
            c = D.part("centres")
            f, y, x = np.meshgrid(np.arange(6), np.arange(cube.size), np.arange(cube.size), indexing="ij")
            want = cube.codes[0][f.reshape(-1), y.reshape(-1), x.reshape(-1), :3].view(np.float16).astype(np.float32)
            assert_same_bits(g0[c], want, cube.name + ": texel centres vs the uploaded texels", D.d[c])
    finally:
        o.close()


def test_debug_environment_refuses_what_it_cannot_do(built):
    from raytracedggx_amd import capi
    c = capi.Context(32, 32)
    try:
        with pytest.raises(capi.RtggxError, match="no environment"):
            c.debug_environment(np.ones((4, 3), np.float32), 0.0)
        cube = EC.random_cube(2, 2)
        c.set_env(capi.FORMAT_RGBA16F, 2, 2, cube.dds_order())
        with pytest.raises(capi.RtggxError, match="rtggx_debug_environment"):
            c.debug_environment(np.zeros((0, 3), np.float32), 0.0)
        assert c.debug_environment(np.ones((1, 3), np.float32), 0.0).shape == (1, 3)
    finally:
        c.close()


# ---- SH ----------------------------------------------------------------------------------------------------------------------------------
def gpu_sh(ctx, cube):
    from raytracedggx_amd import capi
    ctx.set_env(capi.FORMAT_RGBA16F, cube.size, 1, cube.dds_order())
    ctx.transform_sh()
    return ctx.readback(capi.BUF_SH_COEFFS).astype(np.float64).reshape(9, 3)


@pytest.mark.parametrize("size", EC.SH_SIZES)
def test_sh_projection_against_the_model(ctx, size):
    """Signed radiance; 6 s^2 texels fill less than one workgroup, one and a part, whole ones exactly, many and a part."""
    from raytracedggx_amd import capi
    cube = EC.sh_cube(size)
    c, mag = R.sh_project(cube.levels[0], size)
    got = gpu_sh(ctx, cube)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("sh %d: largest |gpu - model| / (2^-23 magnitude) = %.3f" % (size, np.nanmax(np.where(mag > 0, np.abs(got - c) / (EC.SH_BOUND * mag), 0.0))))
    assert (np.abs(got - c) <= EC.SH_BOUND * mag).all(), "sh %d: %s" % (size, (np.abs(got - c) / np.maximum(EC.SH_BOUND * mag, 1e-300)).max())
    # once more on the same cube: the accumulator starts from zero again (the order of the atomics may move the last bit)
    ctx.transform_sh()
    again = ctx.readback(capi.BUF_SH_COEFFS).astype(np.float64).reshape(9, 3)
    assert (np.abs(again - got) <= EC.SH_BOUND * mag).all()
    # the constant cube: L00 = sqrt(4 pi), nothing else
    one = EC.constant_cube(size)
    _, mag1 = R.sh_project(one.levels[0], size)
    want = np.zeros((9, 3)); want[0] = np.sqrt(4.0 * np.pi)
    assert (np.abs(gpu_sh(ctx, one) - want) <= EC.SH_BOUND * mag1).all()


def test_sh_projection_of_each_basis_function(ctx):
    """A 64 x 64 cube holding Y_k returns the k-th unit vector: the axis convention (x, y, z) = (-d.x, -d.y, d.z), the order of the coefficients
    and the basis constants, with neither the oracle nor the model as the witness.  Allowed: the midpoint rule's discretisation error
    (env_cases.basis_answer), what rounding the texels to binary16 moves the sums by (computed, texel by texel), and the SH bound."""
    size = 64
    d, _, _, _ = R.texel_centre_dirs(size)
    w = (d * d).sum(axis=1) ** -1.5
    Y = R.sh_basis(d)
    for k in range(9):
        cube = EC.basis_cube(size, k)
        _, disc = EC.basis_answer(k, size)
        _, mag = R.sh_project(cube.levels[0], size)
        dL = np.abs(cube.levels[0].reshape(-1, 3)[:, 0] - Y[:, k])
        half = (np.abs(Y) * (w * dL)[:, None]).sum(axis=0) * (4.0 * np.pi / w.sum())
        want = np.zeros((9, 3)); want[k] = 1.0
        got = gpu_sh(ctx, cube)
        tol = disc + half[:, None] + EC.SH_BOUND * mag
        assert tol.max() < 5e-3
        assert (np.abs(got - want) <= tol).all(), "Y_%d: %s" % (k, np.abs(got - want).max(axis=1))


# ---- uploads -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,mips", [(6, 3), (12, 3)])
@pytest.mark.parametrize("signed", [False, True], ids=["UF16", "SF16"])
def test_bc6h_levels_whose_side_is_no_multiple_of_four(ctx, size, mips, signed):
    """Random blocks (every mode, reserved ones included).  A level of side 6, 3 or 1 is stored in whole 4 x 4 blocks; the texels beyond the
    level's side must not land anywhere."""
    from raytracedggx_amd import capi
    rng = np.random.default_rng(100 * size + signed)
    per_level = [((EC.side(size, m) + 3) // 4) ** 2 for m in range(mips)]
    blocks = rng.integers(0, 256, (6, sum(per_level), 16), dtype=np.uint8)          # per face: its mip chain
    ctx.set_env(capi.FORMAT_BC6H_SF16 if signed else capi.FORMAT_BC6H_UF16, size, mips, blocks.reshape(-1))
    want = []
    for m in range(mips):
        s, bpr, first = EC.side(size, m), (EC.side(size, m) + 3) // 4, sum(per_level[:m])
        for f in range(6):
            img = np.zeros((4 * bpr, 4 * bpr, 4), np.uint16)
            img[..., 3] = 0x3C00
            for b in range(bpr * bpr):
                img[4 * (b // bpr):4 * (b // bpr) + 4, 4 * (b % bpr):4 * (b % bpr) + 4, :3] = O.bc6h_decode_block(blocks[f, first + b].tobytes(), signed=signed).reshape(4, 4, 3)
            want.append(img[:s, :s].reshape(-1, 4))
    got = ctx.readback(capi.BUF_ENV)
    np.testing.assert_array_equal(got, np.concatenate(want))
    assert (got[:, 3] == 0x3C00).all()


def test_float32_upload_rounds_like_ieee(ctx):
    """RGBA32F -> binary16, round to nearest even, at the edges of the format: half denormals and what lies below them, ties between two
    halves, the overflow threshold, infinities, NaN, both zeros, fp32 denormals."""
    from raytracedggx_amd import capi
    size, mips = 6, 3
    n = 6 * sum(EC.side(size, m) ** 2 for m in range(mips)) * 4
    rng = np.random.default_rng(3)
    h = lambda code: float(np.array([code], np.uint16).view(np.float16)[0])
    edge = [0.0, -0.0, np.inf, -np.inf, np.nan, 65504.0, -65504.0, 65519.996, 65520.0, -65520.0, 65536.0, 1e38, -1e38,
            2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1.0)), np.nextafter(np.float32(2.0 ** -25), np.float32(0.0)), 2.0 ** -26, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24,
            2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(0.0)), 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26,
            1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38,
            1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11, np.nextafter(np.float32(1.0 + 2.0 ** -11), np.float32(2.0)), np.nextafter(np.float32(1.0 + 2.0 ** -11), np.float32(0.0)),
            -(1.0 + 2.0 ** -11), 2047.5, 2048.5, 2049.0, 2051.0, 0.5 * (h(0x7BFE) + h(0x7BFF))]
    edge += [h(c) for c in (1, 2, 0x3FF, 0x400, 0x8001, 0x83FF)] + [0.5 * (h(c) + h(c + 1)) for c in (1, 2, 0x3FE, 0x3FF, 0x400)]
    with np.errstate(over="ignore"):
        src = np.concatenate([np.array(edge, np.float32), rng.uniform(-8.0, 8.0, n - len(edge)).astype(np.float32)])
        # denormal halves at random, both signs
        k = rng.random(n) < 0.2
        k[:len(edge)] = False
        src[k] = (rng.uniform(0.0, 2.0 ** -14, int(k.sum())) * rng.choice([-1.0, 1.0], int(k.sum()))).astype(np.float32)
        src = src[rng.permutation(n)]
        # DDS order in, mip-major out
        faces, at = [], 0
        for f in range(6):
            chain = []
            for m in range(mips):
                s = EC.side(size, m)
                chain.append(src[at:at + 4 * s * s].reshape(s * s, 4)); at += 4 * s * s
            faces.append(chain)
        want = np.concatenate([faces[f][m].astype(np.float16) for m in range(mips) for f in range(6)]).view(np.uint16)
    ctx.set_env(capi.FORMAT_RGBA32F, size, mips, src)
    got = ctx.readback(capi.BUF_ENV)
    nan_w, nan_g = ((want & 0x7C00) == 0x7C00) & ((want & 0x3FF) != 0), ((got & 0x7C00) == 0x7C00) & ((got & 0x3FF) != 0)
    assert nan_w.sum() == 1 and (want == 0x7C00).sum() >= 4 and (want == 0x8000).sum() >= 3      # the edge values are among the texels
    np.testing.assert_array_equal(nan_g, nan_w)
    np.testing.assert_array_equal(np.where(nan_w, 0, got), np.where(nan_w, 0, want))
