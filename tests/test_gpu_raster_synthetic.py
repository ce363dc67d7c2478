"""The HIP visibility pass (visibility.hip, rt_raster.h) against the exact model (tests/raster_ref.py), per pixel, on the synthetic triangles of
tests/raster_cases.py.

Every other test of the rasteriser compares whole rendered frames of real meshes with the CPU oracle, which is the kernel's text a second time:
an error both share passes, and the parts that exist only on the device -- two kernels that share the work at a box of 1024 candidate pixels,
the multiply-shift division, the wave-wide sharing of candidates, two ways of resolving depth, the fallback for a full queue, the tile words
-- meet nothing but a few pixels per triangle of a bunny.  Here coverage and ownership are integer predicates the model decides exactly.

Per case and strip (a bare rtggx_create context: set_mesh for both slots, set_strip, update_frame, render_visibility, readback), on the rows
the pass draws for the strip (the strip and 18 rows on each side, tests/raster_cases.py kernel_rows -- the kernels' rowBegin and rowEnd):
  * the visibility words are the model's on every pixel, the depth codes on every pixel the model does not flag as ambiguous (at most 1 % of a
    case's covered pixels, asserted on the CPU in tests/test_raster_ref_host.py; none in the cases as they stand);
  * both buffers are identical bit for bit to the oracle's, flagged pixels included: the project's standing bar;
  * a second frame in the same context, which draws into the other visibility target, reads back the same words.
Family 9 also renders whole frames (ray tracing, denoiser, tone map) in two contexts, one of them without the tile words: every target is
identical inside the strip.

Which fault each family is there to catch (the ones quoted from the kernel were made once, each in a scratch copy of it, and DESIGN.md
section 3 records which test failed for each):
  1 fill rule            the tie of isTopLeft flipped for horizontal edges; an edge function with the wrong sign or order
  2 watertight meshes    a fill rule that differs between rasterSmall and rasterLarge (a shared edge with one of them on each side)
  3 threshold            the multiply-shift division: a `magic` that is off by one, a product q * magic that leaves 32 bits (boxes of 1 to 3
                         columns and more than 256 rows); boxes of 1023, 1024 and 1025 pixels under either kernel
  4 wave work sharing    prefix[lo + step] <= w turned into <, a prefix sum that drops a lane, a last wave that reads past the end
  5 depth resolve        an atomicMin or a read-min-write that compares only the depth half of the key, z = 1 drawn
  6 clipping             a clipped triangle that stays in rasterSmall, a fan around the wrong vertex, a guard plane out of order
  7 frames and strips    rows of rasterLarge's 64 x 16 blocks counted from 0 instead of the strip's first row, columns beyond a width that is
                         no multiple of 64
  8 full queue           the overflow branch emptied or drawing with another rule
  9 tile words           the tile index taken without - rowBegin (strip (35, 61): the pass's first row is 17), a word that is not set by one
                         of the three places that draw
Two of the mutations tried change no image and no test here fails for them: RT_SMALL_BOX's > turned into >= moves a box of exactly 1024
pixels to the other kernel, which draws the same pixels; best[k] < *dst turned into <= in rasterLarge rewrites a key only with itself (a key
holds the triangle's word, so two fragments never have equal keys).  prefix[lo + step] <= w turned into < was not run: it reads a set-up record
in LDS that nobody wrote.

The overflow case takes about 10 s on the host (building 65800 triangles and their model) and under a second on the GPU; the whole file 8 s there.
NaN and inf are vertex values fed through arithmetic and the full queue is a path the kernel documents as supported: nothing here provokes a fault.
"""
import numpy as np
import pytest

import assets
import raster_cases as RC

pytestmark = pytest.mark.gpu


def device_frames(c, rows, frames=2):
    """[(visibility, depth)] of `frames` consecutive visibility passes of the case in one context."""
    from raytracedggx_amd import capi
    ctx = capi.Context(c.W, c.H)
    try:
        for slot in range(2):
            ctx.set_mesh(slot, *c.mesh(slot))
        ctx.set_strip(*rows)
        out = []
        for _ in range(frames):
            ctx.update_frame(c.constants())
            ctx.render_visibility(); ctx.sync()
            out.append((ctx.readback(capi.BUF_VISIBILITY), ctx.readback(capi.BUF_DEPTH)))
        return out
    finally:
        ctx.close()


@pytest.mark.parametrize("name", RC.names())
def test_kernels_equal_the_model_and_the_oracle(built, name):
    c = RC.case(name)
    m = c.model()
    ovis, odepth = RC.oracle_frame(c)
    for strip in c.strips:
        rows = RC.kernel_rows(strip, c.H)      # everything the pass draws for the strip: its rows and the apron
        s = slice(*rows)
        frames = device_frames(c, strip)
        for f, (vis, depth) in enumerate(frames):
            label = "%s rows %s frame %d" % (name, rows, f)
            print("%s: %d visibility words and %d depth codes differ from the model, %d and %d from the oracle" % (
                label, (vis[s] != m.vis[s]).sum(), (depth[s] != m.depth[s]).sum(), (vis[s] != ovis[s]).sum(), (depth[s] != odepth[s]).sum()))
        for f, (vis, depth) in enumerate(frames):
            label = "%s rows %s frame %d" % (name, rows, f)
            RC.compare(label, vis, depth, m, rows)
            np.testing.assert_array_equal(vis[s], ovis[s], err_msg=label + ": visibility differs from the oracle")
            np.testing.assert_array_equal(depth[s], odepth[s], err_msg=label + ": depth differs from the oracle")
        np.testing.assert_array_equal(frames[0][0][s], frames[1][0][s], err_msg="%s rows %s: the two visibility targets differ" % (name, rows))
        np.testing.assert_array_equal(frames[0][1][s], frames[1][1][s], err_msg="%s rows %s: the two visibility targets differ" % (name, rows))


def _scene_constants(c):
    """The case's constants completed for a whole frame: identity worlds, a camera in front of the NDC cube."""
    fc = c.constants()
    f = fc.view(np.float32)
    for base in (64, 76, 88, 100):                      # Worlds[0], Worlds[1], WorldITs0, WorldIT1 (3 x 4, the last float of WorldIT1 is FrameIndex)
        f[base + 0] = f[base + 5] = f[base + 10] = 1.0
    fc.view(np.uint32)[111] = 0                         # FrameIndex
    f[112:128] = np.eye(4, dtype=np.float32).reshape(-1)   # ProjToWorld
    f[128:132] = (0.0, 0.0, -4.0, 0.0)                  # EyePt
    return fc


@pytest.mark.parametrize("kind", ["small", "large", "overflow"])
def test_tile_words_of_single_pixels_change_no_target(built, kind):
    """Family 9 through the whole frame: one context with the tile words, one without (tile_words(False): every tile counts as drawn), a constant
    1 x 1 environment, both strips, three frames each -- every target identical inside the strip.  A tile that holds one drawn pixel and whose
    word is missing loses that pixel in the context with the words."""
    from raytracedggx_amd import capi
    c = RC.case("9-tiles-%s" % kind)
    targets = (capi.BUF_VISIBILITY, capi.BUF_DEPTH, capi.BUF_NORMAL, capi.BUF_ROUGH_METAL, capi.BUF_VELOCITY, capi.BUF_RT_REFL, capi.BUF_RT_DIFF,
               capi.BUF_FLT_DFF, capi.BUF_TSS0, capi.BUF_TSS1, capi.BUF_BACKBUFFER)
    a, b = capi.Context(c.W, c.H), capi.Context(c.W, c.H)
    try:
        for ctx in (a, b):
            for slot in range(2):
                ctx.set_mesh(slot, *c.mesh(slot))
                ctx.set_material(slot, (0.9, 0.8, 0.7, 1.0), 0.4, 0.5)
            ctx.set_env(capi.FORMAT_RGBA16F, 1, 1, assets.constant_env_rgba16f(1.0))
            ctx.build_as()
        b.tile_words(False)
        m = c.model()
        for rows in c.strips + [(0, c.H)]:
            for f in range(3):
                for ctx in (a, b):
                    if f == 0:
                        ctx.set_strip(*rows)
                    ctx.update_frame(_scene_constants(c))
                    ctx.update_as(); ctx.render_visibility(); ctx.ray_trace(); ctx.denoise(True); ctx.tone_map()
                a.sync(); b.sync()
                s = slice(*rows)
                assert (a.readback(capi.BUF_VISIBILITY)[s] == m.vis[s]).all()
                for bid in targets:
                    np.testing.assert_array_equal(a.readback(bid)[s], b.readback(bid)[s], err_msg="rows %s frame %d buffer %d" % (rows, f, bid))
    finally:
        a.close(); b.close()
