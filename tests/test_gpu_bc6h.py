"""bc6hDecodeKernel (raytracedggx_amd/csrc/env.hip) through rtggx_set_env and a readback of the decoded pyramid, bit for bit against the
exact-integer model of tests/bc6h_cases.py -- not against the oracle, which is the kernel's text once more.  The model's own witnesses are in
tests/test_bc6h_host.py: known answers, and a decoder that shares no text with the project.

Every case of bc6h_cases (all modes, all partitions, the special endpoints and wraps, every index at every texel, all 32 mode ids, random
blocks) travels in cubes whose levels hold 1, 49, 64 and 81 blocks per face: one lane, part of a wave, exactly one 64-lane workgroup, a second
workgroup with a tail.  Each face holds other blocks, so a face or offset slip shows.  One more cube has the chain 36, 18, 9, 4, 2, 1:
levels whose side is no multiple of 4 drop the texels beyond it, and every level sits at its mip-major offset."""
import numpy as np
import pytest

import bc6h_cases as BC

pytestmark = pytest.mark.gpu

SIDES = (4, 28, 32, 36)          # 1, 49, 64, 81 blocks per face
FORMATS = [pytest.param(False, id="UF16"), pytest.param(True, id="SF16")]


@pytest.fixture(scope="module")
def ctx(built):
    from raytracedggx_amd import capi
    c = capi.Context(32, 32)
    yield c
    c.close()


def cubes_of_all_cases():
    """-> [(side, case numbers [6, blocks per face])]: the four sides once each, then side 36 until every case has travelled; the last cube is
    filled up from the start of the list."""
    n, at, out = len(BC.all_cases()[0]), 0, []
    sides = list(SIDES)
    while at < n:
        side = sides.pop(0) if sides else SIDES[-1]
        per_face = (side // 4) ** 2
        out.append((side, (np.arange(at, at + 6 * per_face) % n).reshape(6, per_face)))
        at += 6 * per_face
    return out


def level_image(texels, side):
    """Decoded blocks uint16 [blocks, 16, 3] of one level of one face -> RGBA uint16 [side * side, 4], the texels beyond the side dropped."""
    bpr = (side + 3) // 4
    img = np.zeros((bpr, 4, bpr, 4, 4), np.uint16)
    img[..., :3] = texels.reshape(bpr, bpr, 4, 4, 3).transpose(0, 2, 1, 3, 4)
    img[..., 3] = 0x3C00
    return img.reshape(4 * bpr, 4 * bpr, 4)[:side, :side].reshape(-1, 4)


def report(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return "%s: %d of %d texels differ, first at %d: %s vs the model's %s" % (what, bad.size, len(want), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("signed", FORMATS)
def test_every_case_at_the_launch_shape_edges(ctx, signed):
    from raytracedggx_amd import capi
    blocks, want_all = BC.all_cases()[1], BC.expected(signed)
    travelled = np.zeros(len(blocks), bool)
    cubes = cubes_of_all_cases()
    assert [s for s, _ in cubes[:4]] == list(SIDES) and [(s // 4) ** 2 for s in SIDES] == [1, 49, 64, 81]
    for k, (side, cases) in enumerate(cubes):
        ctx.set_env(capi.FORMAT_BC6H_SF16 if signed else capi.FORMAT_BC6H_UF16, side, 1, blocks[cases].reshape(-1))
        got = ctx.readback(capi.BUF_ENV)
        want = np.concatenate([level_image(want_all[cases[f]], side) for f in range(6)])
        assert got.shape == want.shape and np.array_equal(got, want), report(got, want, "cube %d of side %d" % (k, side))
        assert (got[:, 3] == 0x3C00).all()
        travelled[cases.reshape(-1)] = True
    assert travelled.all()


@pytest.mark.parametrize("signed", FORMATS)
def test_mip_chain_of_side_36(ctx, signed):
    from raytracedggx_amd import capi
    size, mips = 36, 6
    side = [size >> m for m in range(mips)]
    per_level = [((s + 3) // 4) ** 2 for s in side]
    assert side == [36, 18, 9, 4, 2, 1] and per_level == [81, 25, 9, 1, 1, 1]
    blocks, want_all = BC.all_cases()[1], BC.expected(signed)
    cases = (np.arange(6 * sum(per_level)) * 9 % len(blocks)).reshape(6, sum(per_level))      # per face: its chain; every ninth case, all kinds of them
    ctx.set_env(capi.FORMAT_BC6H_SF16 if signed else capi.FORMAT_BC6H_UF16, size, mips, blocks[cases].reshape(-1))
    got = ctx.readback(capi.BUF_ENV)
    want = np.concatenate([level_image(want_all[cases[f, sum(per_level[:m]):sum(per_level[:m + 1])]], side[m]) for m in range(mips) for f in range(6)])
    assert got.shape == want.shape == (6 * sum(s * s for s in side), 4)
    assert np.array_equal(got, want), report(got, want, "chain of side 36")
    assert (got[:, 3] == 0x3C00).all()


@pytest.mark.parametrize("signed", FORMATS)
def test_reserved_modes_are_black_with_alpha_one(ctx, signed):
    """The four reserved ids over random bits and over all ones, among valid blocks in one level of 64 blocks per face."""
    from raytracedggx_amd import capi
    names, blocks = BC.all_cases()
    reserved = np.array([i for i, n in enumerate(names) if any(n.startswith("id %#04x" % r) for r in BC.RESERVED)])
    assert len(reserved) == 36
    cases = np.arange(6 * 64).reshape(6, 64)
    cases[:, ::2] = reserved[np.arange(6 * 32) % len(reserved)].reshape(6, 32)
    ctx.set_env(capi.FORMAT_BC6H_SF16 if signed else capi.FORMAT_BC6H_UF16, 32, 1, blocks[cases].reshape(-1))
    got = ctx.readback(capi.BUF_ENV).reshape(6, 8, 4, 8, 4, 4).transpose(0, 1, 3, 2, 4, 5).reshape(6, 64, 16, 4)
    assert (got[:, ::2, :, :3] == 0).all() and (got[..., 3] == 0x3C00).all()
    np.testing.assert_array_equal(got[..., :3], BC.expected(signed)[cases])
