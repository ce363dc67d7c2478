"""Progressive accumulation on the GPU (rtggx_set_accumulation, -accumulate N; include/rtggx.h, DESIGN.md "Progressive accumulation").  Its
parity status: no counterpart in the reference; the sums, the count and the presented mean image are pinned bit for bit to the numpy
restatement (tests/accum_ref.py) fed the device's own per-frame words, which the rest of the suite pins to the oracle.  Every pixel of
every buffer is compared.  The small frame is 100x54: the width no multiple of 16 or 64, the height no multiple of 16."""
import numpy as np
import pytest

import accum_ref as AR
import assets
import gpu_support as G

pytestmark = pytest.mark.gpu

IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS


def _words(a):
    """The frame just rendered: (RayTracingOut0, RayTracingOut1, visibility); synchronises."""
    from raytracedggx_amd import capi
    c = a.context
    return c.readback(capi.BUF_RT_REFL), c.readback(capi.BUF_RT_DIFF), c.readback(capi.BUF_VISIBILITY)


def _sums(a):
    from raytracedggx_amd import capi
    return a.context.readback(capi.BUF_ACC_REFL), a.context.readback(capi.BUF_ACC_DIFF), a.context.accumulated_frames()


def _assert_sums(got, want, label):
    """want: an AR.Accumulator or a (refl, diff, frames) triple."""
    if isinstance(want, AR.Accumulator):
        want = (want.refl, want.diff, want.frames)
    assert got[2] == want[2], "%s: %d frames counted, %d expected" % (label, got[2], want[2])
    for name, g, w in (("ACC_REFL", got[0], want[0]), ("ACC_DIFF", got[1], want[1])):
        bad = ~AR.same_bits(g, w)
        assert not bad.any(), "%s: %s differs at %d of %d values, first at %s: %r vs %r" % (
            label, name, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), g[bad][0], w[bad][0])


def _restated_run(a, metallic, frames, acc=None):
    """`frames` frames of an accumulating app, each read back (synchronising) and added to the restatement."""
    acc = acc or AR.Accumulator(a.height, a.width)
    for _ in range(frames):
        G.frame(a)
        refl, diff, vis = _words(a)
        acc.add(refl, diff, vis, metallic)
    return acc


# ---- 1. restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,metallic,extra", [
    ("bunny.obj", (1.0, 1.0), []), ("bunny.obj", (0.25, 0.5), []), ("bunny.obj", (1.0, 0.75), []),
    ("bunny.obj", (0.25, 0.5), ["-vndf"]), ("bunny.obj", (0.25, 0.5), ["-spp", 4, "-recursion", 2]), ("dragon.obj", (0.25, 0.5), [])],
    ids=["metal", "diffuse", "metal-ground", "vndf", "spp4-depth2", "dragon"])
def test_sums_equal_the_restatement(built, mesh, metallic, extra):
    """100x54, 6 frames: RTGGX_BUF_ACC_REFL, _ACC_DIFF and the count against the restatement after every frame, bit for bit."""
    a = G.app(100, 54, ["-metallic", metallic[0], metallic[1]] + extra, mesh=mesh)
    try:
        a.context.set_accumulation(True)
        assert a.context.accumulated_frames() == 0
        acc = AR.Accumulator(54, 100)
        for f in range(6):
            _restated_run(a, metallic, 1, acc)
            _assert_sums(_sums(a), acc, "%s %s frame %d" % (mesh, extra, f))
        assert acc.refl[..., :3].any() and acc.refl[..., 3].any()
        covered = AR.diffuse_mask(_words(a)[2], metallic)
        assert covered.any() == (min(metallic) < 1.0) == bool(acc.diff.any())
    finally:
        a.OnDestroy()


# ---- 2. accumulating changes nothing else ---------------------------------------------------------------------------------------------
def test_accumulating_changes_no_other_buffer(built):
    """320x180, 8 frames: an accumulating context, one that enabled and disabled before its first frame, one that never heard of it --
    G-buffer, raw images, filtered images, both TemporalSSOut, back buffer and ray count, every frame."""
    extra = ["-metallic", 0.25, 0.5]
    a, b, c = G.app(320, 180, extra), G.app(320, 180, extra), G.app(320, 180, extra)
    try:
        a.context.set_accumulation(True)
        b.context.set_accumulation(True); b.context.set_accumulation(False)
        for f in range(8):
            for x in (a, b, c):
                G.frame(x)
            ic = G.images(c, IMAGES)
            G.assert_same(G.images(a, IMAGES), ic, "accumulating, frame %d" % f)
            G.assert_same(G.images(b, IMAGES), ic, "enabled and disabled, frame %d" % f)
        assert a.context.accumulated_frames() == 8 and b.context.accumulated_frames() == 0
        assert not _sums(b)[0].any() and not _sums(b)[1].any(), "a context that never accumulated a frame holds zero sums"
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


# ---- 3. scheduling ---------------------------------------------------------------------------------------------------------------------
SCHED_EXTRA = ["-metallic", 1.0, 0.5]


@pytest.fixture(scope="module")
def synchronised_twin(built):
    """16 frames at 320x180 with a synchronising readback after each: its sums (checked against the restatement), shared by the variants."""
    a = G.app(320, 180, SCHED_EXTRA)
    try:
        a.context.set_accumulation(True)
        acc = _restated_run(a, (1.0, 0.5), 16)
        got = _sums(a)
        _assert_sums(got, acc, "synchronised twin")
        return got
    finally:
        a.OnDestroy()


@pytest.mark.parametrize("variant", ["small-placement", "full-size-placement", "sync-flag", "caller-stream"])
def test_free_running_frames_accumulate_what_synchronised_ones_do(built, synchronised_twin, variant):
    import torch
    b = G.app(320, 180, SCHED_EXTRA + (["-sync"] if variant == "sync-flag" else []))
    stream = torch.cuda.Stream() if variant == "caller-stream" else None
    try:
        if variant == "small-placement":
            b.context.placement(1)
        if variant == "full-size-placement":
            b.context.placement(0)
        if stream is not None:
            b.context.set_stream(stream.cuda_stream)
        b.context.set_accumulation(True)
        for f in range(16):
            G.frame(b)
        _assert_sums(_sums(b), synchronised_twin, variant)
        if variant == "small-placement":
            assert b.context.placement(1)[1]["shade"] == "B", "small launches shade on the traversal's stream"
        if variant == "full-size-placement":
            assert b.context.placement(0)[1]["shade"] == "main"
        if stream is not None:
            b.context.set_stream(0)
    finally:
        b.OnDestroy()


# ---- 4. still sky and tile words ------------------------------------------------------------------------------------------------------
def test_still_sky_tiles_are_accumulated_like_any_other(built):
    """320x180, still camera, 12 frames (past the still-sky threshold: ray generation leaves the sky tiles alone, and the kernel adds the
    words they hold all the same): the restatement, and contexts with the still sky and the tile words off."""
    extra = ["-metallic", 1.0, 0.5]
    a, b, c = G.app(320, 180, extra), G.app(320, 180, extra), G.app(320, 180, extra)
    try:
        b.context.static_sky(False)
        c.context.tile_words(False)
        for x in (a, b, c):
            x.context.set_accumulation(True)
        acc = AR.Accumulator(180, 320)
        for f in range(12):
            G.frame(b); G.frame(c)
            _restated_run(a, (1.0, 0.5), 1, acc)
        runs, threshold = a.context.sky_runs()
        assert (runs >= threshold).any(), "no sky tile is being left alone: the test does not test what it says"
        sa = _sums(a)
        _assert_sums(sa, acc, "still sky on")
        _assert_sums(_sums(b), sa, "still sky off")
        _assert_sums(_sums(c), sa, "tile words off")
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


# ---- 5. strips ------------------------------------------------------------------------------------------------------------------------
def test_a_strip_accumulates_its_own_rows(built):
    extra = ["-metallic", 0.25, 0.5]
    a, b = G.app(100, 54, extra), G.app(100, 54, extra)
    try:
        b.context.set_strip(10, 37)
        a.context.set_accumulation(True); b.context.set_accumulation(True)
        for f in range(3):
            G.frame(a); G.frame(b)
        ra, da, na = _sums(a)
        rb, db, nb = _sums(b)
        assert na == nb == 3
        for name, whole, strip in (("ACC_REFL", ra, rb), ("ACC_DIFF", da, db)):
            assert AR.same_bits(whole[10:37], strip[10:37]).all(), name + ": the strip's rows differ from the whole frame's"
            assert not strip[:10].any() and not strip[37:].any(), name + ": rows outside the strip were touched"
        assert rb[10:37].any() and db[10:37].any()
    finally:
        a.OnDestroy(); b.OnDestroy()


# ---- 6. control ------------------------------------------------------------------------------------------------------------------------
def test_reset_disable_and_a_material_change_follow_the_restatement(built):
    a = G.app(100, 54)      # all metal: no diffuse path yet
    try:
        ctx = a.context
        ctx.set_accumulation(True)
        acc = _restated_run(a, (1.0, 1.0), 2)
        _assert_sums(_sums(a), acc, "two frames")
        assert not acc.diff.any()
        # a reset in mid-run, enqueued behind a frame nobody has waited for
        G.frame(a); ctx.reset_accumulation()
        assert ctx.accumulated_frames() == 0
        acc.reset()
        _restated_run(a, (1.0, 1.0), 1, acc)
        _assert_sums(_sums(a), acc, "one frame after the reset")
        # off for two frames: sums and count stay
        ctx.set_accumulation(False)
        for f in range(2):
            G.frame(a)
        _assert_sums(_sums(a), acc, "off for two frames")
        ctx.set_accumulation(True)      # enabling does not reset
        _restated_run(a, (1.0, 1.0), 1, acc)
        _assert_sums(_sums(a), acc, "on again")
        assert not _sums(a)[1].any(), "no frame had a diffuse path so far"
        # the model's metallic from 1 to 0.5: from here on RayTracingOut1 is accumulated under the model
        ctx.set_metallic(1, 0.5)
        _restated_run(a, (1.0, 0.5), 2, acc)
        got = _sums(a)
        _assert_sums(got, acc, "after the material change")
        assert got[2] == 4 and got[1].any()
        vis = _words(a)[2]
        assert got[1][AR.diffuse_mask(vis, (1.0, 0.5))].all(axis=-1).any(), "the model's pixels hold the two diffuse frames"
    finally:
        a.OnDestroy()


# ---- 7. present ------------------------------------------------------------------------------------------------------------------------
def test_present_writes_the_mean_and_its_tone_map_and_nothing_else(built):
    from raytracedggx_amd import capi
    extra, metallic = ["-metallic", 0.25, 0.5], (0.25, 0.5)
    a, twin, fresh = G.app(100, 54, extra), G.app(100, 54, extra), G.app(100, 54, extra)
    try:
        a.context.set_accumulation(True); twin.context.set_accumulation(True)
        acc = AR.Accumulator(54, 100)
        for f in range(3):
            _restated_run(a, metallic, 1, acc); G.frame(twin)
        before = G.images(a, IMAGES)
        a.context.present_accumulation()
        converged = a.context.readback(capi.BUF_CONVERGED)
        np.testing.assert_array_equal(converged, acc.converged(), err_msg="RTGGX_BUF_CONVERGED against the restatement")
        assert (converged >> np.uint64(48) == 0x3C00).all()      # alpha 1.0
        # the back buffer: the frame's own tone map over that image
        G.frame(fresh)
        fresh.context.upload(capi.BUF_TSS0 + fresh.context.frame_parity(), converged)
        fresh.context.tone_map()
        back = a.context.readback(capi.BUF_BACKBUFFER)
        np.testing.assert_array_equal(back, fresh.context.readback(capi.BUF_BACKBUFFER), err_msg="the presented back buffer")
        assert (back != before["back"]).any()
        after = G.images(a, IMAGES)
        for k in before:
            if k != "back":
                np.testing.assert_array_equal(after[k], before[k], err_msg="present touched " + k)
        _assert_sums(_sums(a), acc, "present leaves the sums alone")
        # the frames after it
        for f in range(3):
            _restated_run(a, metallic, 1, acc); G.frame(twin)
            G.assert_same(G.images(a, IMAGES), G.images(twin, IMAGES), "frame %d after the present" % f)
        _assert_sums(_sums(a), acc, "six frames")
        _assert_sums(_sums(twin), acc, "the twin's six frames")
        a.context.present_accumulation()
        np.testing.assert_array_equal(a.context.readback(capi.BUF_CONVERGED), acc.converged(), err_msg="the second present")
    finally:
        a.OnDestroy(); twin.OnDestroy(); fresh.OnDestroy()


def test_save_converged_writes_the_tone_mapped_mean_and_reports_it(built, tmp_path, capfd):
    """-accumulate N through app.py (a run driven from Python has no -frames: on from the first frame) and RayTracedGGX::SaveConverged: the
    present, the PNG -- the tone map of RTGGX_BUF_CONVERGED, which is the restatement's --, and the line with the count and the error."""
    import os
    import re
    import sys
    from raytracedggx_amd import capi
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import imgdiff
    extra, metallic = ["-metallic", 0.25, 0.5], (0.25, 0.5)
    a, fresh = G.app(100, 54, extra + ["-accumulate", 4]), G.app(100, 54, extra)
    try:
        acc = _restated_run(a, metallic, 3)
        path = str(tmp_path / "still_converged.png")
        capfd.readouterr()
        assert a.save_converged(path)
        out = capfd.readouterr().out
        m = re.search(r"accumulated 3 frames: mean relative standard error of Y over covered pixels, reflection ([0-9.]+), diffuse ([0-9.]+)", out)
        assert m and 0.0 < float(m.group(1)) < 10.0 and 0.0 < float(m.group(2)) < 10.0, out
        converged = a.context.readback(capi.BUF_CONVERGED)
        np.testing.assert_array_equal(converged, acc.converged())
        G.frame(fresh)
        fresh.context.upload(capi.BUF_TSS0 + fresh.context.frame_parity(), converged)
        fresh.context.tone_map()
        back = fresh.context.readback(capi.BUF_BACKBUFFER)
        np.testing.assert_array_equal(imgdiff.load(path), back.view(np.uint8).reshape(54, 100, 4)[..., :3])
        _assert_sums(_sums(a), acc, "after SaveConverged")
    finally:
        a.OnDestroy(); fresh.OnDestroy()
    b = G.app(100, 54)      # nothing accumulated: refused, no file
    try:
        G.frame(b)
        assert not b.save_converged(str(tmp_path / "none.png")) and not os.path.exists(str(tmp_path / "none.png"))
    finally:
        b.OnDestroy()


def test_non_finite_words_add_as_they_are(built):
    """An environment of +infinity: every background word, and the word of every reflection ray that misses, carries the exponent-31 code.
    The sums take them as the restatement does (infinity, and NaN where 0 x infinity arose; a NaN's payload is not compared)."""
    from raytracedggx_amd import capi
    a = G.app(100, 54, mesh="triangle.obj")
    try:
        a.context.set_env(capi.FORMAT_RGBA16F, 1, 1, assets.constant_env_rgba16f(np.inf))
        a.context.set_accumulation(True)
        acc = _restated_run(a, (1.0, 1.0), 3)
        got = _sums(a)
        _assert_sums(got, acc, "infinite environment")
        sky = _words(a)[2] == 0
        assert sky.any() and np.isinf(got[0][sky]).all()
    finally:
        a.OnDestroy()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_rendering_the_same_frames(built):
    from raytracedggx_amd import capi
    new_buffers = (capi.BUF_ACC_REFL, capi.BUF_ACC_DIFF, capi.BUF_CONVERGED)
    # rate 4 on an accumulating context; present at n = 0; the new buffers before the first enable
    a, twin = G.app(320, 180, ["-metallic", 1.0, 0.5]), G.app(320, 180, ["-metallic", 1.0, 0.5])
    try:
        for bid in new_buffers:
            for call in (a.context.readback, a.context.buffer_size, a.context.buffer_ptr):
                with pytest.raises(capi.RtggxError, match="rtggx_set_accumulation"):
                    call(bid)
        with pytest.raises(capi.RtggxError, match="rtggx_present_accumulation"):
            a.context.present_accumulation()      # never enabled
        a.context.set_accumulation(True); twin.context.set_accumulation(True)
        with pytest.raises(capi.RtggxError, match="rtggx_present_accumulation"):
            a.context.present_accumulation()      # n = 0
        for f in range(3):
            with pytest.raises(capi.RtggxError, match="rtggx_set_ray_rate"):
                a.context.set_ray_rate(4)
            G.frame(a); G.frame(twin)
            G.assert_same(G.images(a, IMAGES), G.images(twin, IMAGES), "accumulating, rate 4 refused, frame %d" % f)
        _assert_sums(_sums(a), _sums(twin), "accumulating, rate 4 refused")
        assert a.context.buffer_size(capi.BUF_ACC_REFL) == 320 * 180 * 16 and a.context.buffer_size(capi.BUF_CONVERGED) == 320 * 180 * 8
        assert a.context.buffer_ptr(capi.BUF_ACC_DIFF) != 0
    finally:
        a.OnDestroy(); twin.OnDestroy()
    # accumulation on a rate-4 context
    a, twin = G.app(320, 180, ["-rayrate", 4]), G.app(320, 180, ["-rayrate", 4])
    try:
        for f in range(3):
            with pytest.raises(capi.RtggxError, match="rtggx_set_accumulation"):
                a.context.set_accumulation(True)
            G.frame(a); G.frame(twin)
            G.assert_same(G.images(a, IMAGES), G.images(twin, IMAGES), "rate 4, accumulation refused, frame %d" % f)
        assert a.context.accumulated_frames() == 0
        with pytest.raises(capi.RtggxError):
            a.context.readback(capi.BUF_ACC_REFL)      # the refused enable allocated nothing
    finally:
        a.OnDestroy(); twin.OnDestroy()
    # present on a strip
    a, twin = G.app(100, 54), G.app(100, 54)
    try:
        for x in (a, twin):
            x.context.set_strip(10, 37); x.context.set_accumulation(True)
        for f in range(2):
            G.frame(a); G.frame(twin)
            with pytest.raises(capi.RtggxError, match="rtggx_present_accumulation"):
                a.context.present_accumulation()
            ia, it = G.images(a, IMAGES), G.images(twin, IMAGES)
            for k in ("refl", "diff", "tss0", "tss1", "back"):
                np.testing.assert_array_equal(ia[k][10:37], it[k][10:37], err_msg="strip, present refused, frame %d: %s" % (f, k))
        _assert_sums(_sums(a), _sums(twin), "strip, present refused")
        assert not a.context.readback(capi.BUF_CONVERGED).any()
    finally:
        a.OnDestroy(); twin.OnDestroy()
