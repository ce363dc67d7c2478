"""The staging of the tiled denoise kernels (denoise.hip: spatialTiledKernel, stageTemporalTiles) at the sizes where it can go wrong.

Those kernels issue every global load of a thread's texels before they use one, at addresses CLAMPED into the frame and into the tile's
texel count, and select afterwards what a texel outside them stages: the zeros D3D returns, never the texel its address was clamped to.
What can go wrong is therefore at the frame's edges, in ragged blocks and in the part of a tile no thread's second or third texel reaches:
  * frames narrower than an apron (17 x 5: one ragged block, every tap row leaves the frame on both sides), a second H block that lies
    partly outside with a height that is no multiple of the V block (80 x 24), several blocks each way (200 x 37);
  * tiles with a surface everywhere, with none (a block that returns after its loads were issued, before it writes LDS) and mixed ones;
  * centre normals with nx + ny + nz < -1.19 ON each of the four edges: a tap outside the frame reads the normal (-1, -1, -1), its 512th power
    overflows, 0 x inf = NaN (denoise.hip tapWeight) -- a texel that kept the clamped texel's normal would give a finite weight instead;
  * a strip whose rows are not tile-aligned (rows 5 .. 30 of 80 x 37): the own pixel is clamped against rowEnd, the tile's texels against
    the frame's height, and the tile words are counted from the strip's first G-buffer row;
  * the temporal pass and the fused temporal + tone-map kernel at 67 x 7 and 130 x 18 with reprojections that leave the frame over each edge.
The direct-access variant of the spatial passes (spatialDirectKernel) fetches every tap behind its own bounds check: the tiled variant must
give its words, all of them.  The temporal results are held to the float64 model (tests/denoise_ref.py) with the bounds of
tests/test_gpu_denoise_synthetic.py -- recorded floor times margin; the floor of a case of this file is measured on the CPU oracle when the
test runs, by the function that recorded the others (test_denoise_ref_host.measure) -- and the fused kernel to the two-kernel path bit for bit.
After rtggx_upload the tiles' words read "unknown", as in the other synthetic tests: the tile-word early-outs are not under test here.
NaN and inf are values fed through arithmetic; nothing here provokes a fault.
"""
import numpy as np
import pytest

import denoise_cases as DC
import denoise_ref as R
import test_denoise_ref_host as HOST
import test_gpu_denoise_synthetic as SYN

pytestmark = pytest.mark.gpu

FAR = (-0.58, -0.58, -0.575)      # nx + ny + nz = -1.735, |n|^2 = 1.0034 (denoise_cases._normals)
BUFFERS = ("flt_rfl", "flt_dff", "tss", "bb")
_CASES, _RECORDED = {}, {}


def edge_pixels(W, H):
    """(x, y) of one pixel on the left, right, top and bottom edge."""
    return ((0, H // 2), (W - 1, max(H // 2 - 1, 0)), (W // 2, 0), (min(W // 2 + 3, W - 1), H - 1))


def spatial_case(W, H, seed, strips=()):
    """Surface, sky and mixed tiles, half the texels outside the diffuse passes, and the four edge normals."""
    key = ("spatial", W, H)
    if key not in _CASES:
        c = DC.Case("staging_%dx%d" % (W, H), W, H, seed, metallic=(1.0, 0.5))
        col = (c.xs // 16).astype(np.int64) % 4
        sky = (col == 2) | ((c.xs >= 64) & (c.xs < 128) & (c.ys >= 8) & (c.ys < 24))      # whole V blocks, and a whole H block at 200 x 37
        mixed = (col == 1) & (c.rng.random((H, W)) < 0.4)
        c.hole(sky | mixed | ((c.xs % 7 == 3) & (c.ys % 3 == 1)))
        for x, y in edge_pixels(W, H):
            at = (c.xs == x) & (c.ys == y)
            c.set_normal(at, FAR)
            c.acode = np.where(at, 3, c.acode).astype(np.uint32)
        c.strips = list(strips)
        _CASES[key] = c
    return _CASES[key]


def temporal_case(W, H, seed):
    """Reprojections of several pixels that leave the frame over each of the four edges, sub-pixel ones elsewhere, holes."""
    key = ("temporal", W, H)
    if key not in _CASES:
        c = DC.Case("staging_temporal_%dx%d" % (W, H), W, H, seed)
        c.hole(c.rng.random((H, W)) < 0.1)
        v = c.vel.astype(np.float64)
        band = lambda m, vx, vy: np.where(m[..., None], np.array([vx, vy]), v)
        v = band(c.xs < 3, 2.5 / W, 0.0)                                     # uv - v: to the left of the frame
        v = band(c.xs >= W - 3, -2.5 / W, 0.0)
        v = band((c.ys < 2) & (c.xs >= 3) & (c.xs < W - 3), 0.0, 2.5 / H)
        v = band((c.ys >= H - 2) & (c.xs >= 3) & (c.xs < W - 3), 0.0, -2.5 / H)
        c.vel = v.astype(np.float16)
        _CASES[key] = c
    return _CASES[key]


def recorded_with(case):
    """The recorded floor plus this case's own entry, measured now on the CPU oracle (once per case)."""
    if case.name not in _RECORDED:
        doc = SYN.floor()
        doc["cases"][case.name] = {v: HOST.measure(case, v) for v in HOST.VARIANTS}
        _RECORDED[case.name] = doc
    return _RECORDED[case.name]


def assert_words_equal(a, b, label, rows=None):
    rs = slice(None) if rows is None else slice(*rows)
    for k in BUFFERS:
        np.testing.assert_array_equal(a[k][rs], b[k][rs], err_msg="%s: %s" % (label, k))


@pytest.mark.parametrize("W,H", [(17, 5), (80, 24), (200, 37)])
def test_tiled_passes_give_the_direct_passes_words(built, W, H):
    """All four modes of spatialTiledKernel (the materials launch the diffuse passes) against spatialDirectKernel, word for word, and the NaN
    pixels the same set -- with the four edge pixels in it."""
    case = spatial_case(W, H, 7000 + W)
    assert min(m for _, m in case.materials) < 1.0 and (case.metal < 255).any() and (case.metal == 255).any()
    _, direct = SYN.run_device(case, False, False)
    _, tiled = SYN.run_device(case, True, False)
    for k in ("flt_rfl", "flt_dff"):
        d, t = R.from_f16_words(direct[k]), R.from_f16_words(tiled[k])
        np.testing.assert_array_equal(np.isnan(t), np.isnan(d), err_msg="%s: NaN pixels of %s" % (case.name, k))
        for x, y in edge_pixels(W, H):
            assert np.isnan(t[y, x, :3]).all(), "%s: %s at the edge pixel (%d, %d) is not NaN: %s" % (case.name, k, x, y, t[y, x])
        assert np.isfinite(t[..., :3]).any(), "%s: no finite pixel left in %s" % (case.name, k)
    assert_words_equal(tiled, direct, case.name + ": tiled against direct")
    # a pixel without a surface passes the raw texel through; sky tiles and mixed ones are there
    b = case.buffers()
    assert ((b["normal"] >> 30) == 0).any() and ((b["normal"] >> 30) != 0).any()


def test_strip_with_rows_off_the_tile_grid(built):
    """Rows 5 .. 30 of 80 x 37: the rows inside the strip, tiled against direct in both temporal paths word for word, and against the model."""
    strip = (5, 30)
    case = spatial_case(80, 37, 7100, strips=[strip])
    b, m = HOST.model_chain(case)
    recorded = recorded_with(case)
    runs = {mode: SYN.run_device(case, shared_mem, fuse, strip=strip)[1] for mode, shared_mem, fuse in SYN.MODES}
    for mode in ("sharedmem", "sharedmem+fused"):
        label = "%s rows %d-%d [%s]" % (case.name, strip[0], strip[1], mode)
        assert_words_equal(runs[mode], runs["direct"], label + " against [direct]", rows=strip)
        SYN.assert_bounds(label, case.name, SYN.check_against_model(case, label, b, m, runs[mode], rows=strip), recorded)
    assert_words_equal(runs["direct+fused"], runs["direct"], case.name + " [direct+fused] against [direct]", rows=strip)


@pytest.mark.parametrize("W,H", [(67, 7), (130, 18)])
def test_temporal_staging_against_the_model(built, W, H):
    """temporalKernel and temporalToneKernel (both stage through stageTemporalTiles): each against the float64 model fed the device's own
    input words, with the synthetic tests' bounds; the fused kernel's TemporalSSOut and back buffer equal to the two kernels', bit for bit."""
    case = temporal_case(W, H, 7200 + W)
    vel = case.vel.astype(np.float64)
    assert (vel[:, 0, 0] * W > 2).all() and (vel[:, -1, 0] * W < -2).all() and (vel[0, 5:-5, 1] * H > 2).all() and (vel[-1, 5:-5, 1] * H < -2).all()
    b, m = HOST.model_chain(case)
    recorded = recorded_with(case)
    runs = {}
    for mode, fuse in (("sharedmem", False), ("sharedmem+fused", True)):
        _, runs[mode] = SYN.run_device(case, True, fuse)
        label = "%s [%s]" % (case.name, mode)
        SYN.assert_bounds(label, case.name, SYN.check_against_model(case, label, b, m, runs[mode]), recorded)
    assert_words_equal(runs["sharedmem+fused"], runs["sharedmem"], case.name + ": fused against the two kernels")
