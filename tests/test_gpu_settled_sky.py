"""Settled sky (denoise.hip temporalKernel, toneMapKernel; rtggx_context.h rtggx_context::settled): over sky that has
stopped changing the temporal pass leaves a 64x4 block alone once the block and its eight neighbours stored, in the frame before, the very
bits the other history image held, and the tone map leaves a 64x16 block alone over such blocks.  Nothing a frame computes may change: one
context with the feature beside one with rtggx_debug_settled_sky(ctx, 0), bit for bit after every frame; and the blocks left alone are
exactly the ones the rule names.  320x180 is a small launch, whose tone map the library fuses into the temporal pass: both contexts pin
the two-kernel path, which is the one the feature lives in."""
import numpy as np
import pytest

import assets

pytestmark = pytest.mark.gpu

W, H = 320, 180
STILL = 24      # frames of a still stretch: the history alpha counts up for about 16 of them, and every input set (4) goes by after that
SETTLED, SKIPPED = 1, 2


def _pair():
    from raytracedggx_amd import app
    args = ["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", W, "-height", H, "-sharedmem", "-dt", 0.25]
    a, b = app.RayTracedGGX(args), app.RayTracedGGX(args)
    for x in (a, b):
        x.context.fuse_tone_map(False)
    return a, b


def _skipped(ctx):
    """Blocks the most recent temporal pass left alone: bit 1 of the newest array's words that count under the current epoch."""
    words, epoch = ctx.settled_words()
    w = words[ctx.frame_parity()]
    return int((((w >> 8) == epoch) & ((w & SKIPPED) != 0)).sum())


def test_settled_sky_changes_no_buffer_through_every_event_that_unsettles_it(built):
    """Context A with the feature, context B with settled_sky(False); FilteredOut1, both history images and the back buffer compared after
    every frame.  Still stretches of 24 frames between the events that must unsettle every block or keep a pass from leaving any alone:
    a camera drag over four frames, the fused tone map on and off, a strip of rows 37-150 and back, a frame without the denoiser, a frame
    that denoises and presents the accumulation mean instead, an upload into the current history image and one into the back buffer
    between the denoiser and the tone map, static_sky off and on, ray rate 4 and back, a constant environment.  After each still stretch
    blocks are left alone (the comparison is not vacuous); in the first frame after every event that starts a new epoch none is.
    The test can fail: built with -DRT_SETTLED_NO_COMPARE (denoise.hip temporalKernel: a block whose window is sky is marked settled
    without comparing; `EXTRA=-DRT_SETTLED_NO_COMPARE` in the environment of the build) it fails while the history alpha still counts up, in the
    third frame of the first still stretch already -- `start, still 2 (frame 2): buffer 11`, 7 168 of 57 600 texels of the back buffer: blocks
    marked settled in frame 1 were left alone in frame 2.  Run once that way on an MI355X."""
    from raytracedggx_amd import capi
    a, b = _pair()
    targets = (capi.BUF_FLT_DFF, capi.BUF_TSS0, capi.BUF_TSS1, capi.BUF_BACKBUFFER)
    count = [0]

    def check(label):
        a.context.sync(); b.context.sync()
        for bid in targets:
            np.testing.assert_array_equal(a.context.readback(bid), b.context.readback(bid), err_msg="%s (frame %d): buffer %d" % (label, count[0], bid))
        count[0] += 1

    def frame(label, before=None, render=None):
        for x in (a, b):
            if before is not None:
                before(x)
            x.OnUpdate()
            if render is not None:
                render(x.context)
            else:
                x.OnRender()
        check(label)

    def still(label, n=STILL, settles=True):
        for k in range(n):
            frame("%s, still %d" % (label, k))
        if settles:
            n = _skipped(a.context)
            print("%s: %d blocks left alone" % (label, n))
            assert n > 0, label

    def new_epoch(label, before=None, render=None):
        frame(label, before, render)
        assert _skipped(a.context) == 0, label

    def upload_before_tone_map(which):
        def render(c):
            c.render_visibility(); c.update_as(); c.ray_trace(); c.denoise(True); c.sync()
            bid = capi.BUF_TSS0 + c.frame_parity() if which == "history" else capi.BUF_BACKBUFFER
            image = c.readback(bid)
            c.upload(bid, image ^ image.dtype.type(1))
            c.tone_map()
        return render

    try:
        b.context.settled_sky(False)
        still("start")
        # a camera drag over four frames (the events of test_scripted_camera_and_material_track)
        new_epoch("drag 1", lambda x: (x.OnLButtonDown(160, 90), x.OnMouseMove(150, 86)))
        new_epoch("drag 2", lambda x: x.OnMouseMove(128, 80))
        new_epoch("drag 3", lambda x: (x.OnMouseMove(100, 84), x.OnMouseWheel(2.0)))
        new_epoch("drag 4", lambda x: (x.OnLButtonUp(0, 0), x.OnMouseMove(10, 10)))
        still("after the drag")
        # the temporal pass and the tone map as one kernel, and as two again
        frame("fused", lambda x: x.context.fuse_tone_map(True))
        still("fused", 2, settles=False)
        frame("two kernels", lambda x: x.context.fuse_tone_map(False))
        still("two kernels again")
        # a strip of rows 37-150 and back to the whole frame
        new_epoch("strip", lambda x: x.context.set_strip(37, 150))
        still("strip", 4, settles=False)
        new_epoch("whole frame", lambda x: x.context.set_strip(0, H))
        still("whole frame")
        # a frame without the denoiser
        frame("no denoise", render=lambda c: (c.render_visibility(), c.update_as(), c.ray_trace(), c.tone_map()))
        still("after no denoise")
        # a frame that denoises and presents the accumulation mean: the tone map reads another image than the history
        frame("accumulation on", lambda x: x.context.set_accumulation(True))
        frame("present", render=lambda c: (c.render_visibility(), c.update_as(), c.ray_trace(), c.denoise(True), c.present_accumulation()))
        frame("accumulation off", lambda x: x.context.set_accumulation(False))
        still("after the accumulation mean")
        # uploads between the denoiser and the tone map: into the history image the pass has just written, into the back buffer
        new_epoch("upload into the history", render=upload_before_tone_map("history"))
        still("after the upload into the history")
        new_epoch("upload into the back buffer", render=upload_before_tone_map("back buffer"))
        still("after the upload into the back buffer")
        # still sky off and on
        new_epoch("static sky off", lambda x: x.context.static_sky(False))
        still("static sky off", 4, settles=False)
        new_epoch("static sky on", lambda x: x.context.static_sky(True))
        still("static sky on")
        # one ray per 2x2 quad and back
        new_epoch("rate 4", lambda x: x.context.set_ray_rate(4))
        still("rate 4", 6, settles=False)
        new_epoch("rate 1", lambda x: x.context.set_ray_rate(1))
        still("rate 1")
        # a constant environment
        env = assets.constant_env_rgba16f(0.5)
        new_epoch("environment", lambda x: x.context.set_env(capi.FORMAT_RGBA16F, 1, 1, env))
        still("after the environment")
    finally:
        a.OnDestroy(); b.OnDestroy()


def _rule(runs, words_before, epoch):
    """The rule, restated: a block is left alone when every 16x16 tile its 66x6 window touches (clamped to the frame) has a run of at
    least 1 under the epoch, and the block and its eight neighbours were settled under the epoch in the frame before; a neighbour outside
    the grid counts as settled."""
    by_n, bx_n = words_before.shape
    settled = np.ones((by_n + 2, bx_n + 2), bool)
    settled[1:-1, 1:-1] = (words_before & ~np.uint32(SKIPPED)) == np.uint32((epoch << 8) | SETTLED)
    skip = np.zeros((by_n, bx_n), bool)
    for by in range(by_n):
        for bx in range(bx_n):
            tx0, tx1 = max(bx * 64 - 1, 0) // 16, min(bx * 64 + 64, W - 1) // 16
            ty0, ty1 = max(by * 4 - 1, 0) // 16, min(by * 4 + 4, H - 1) // 16
            window_sky = bool((runs[ty0:ty1 + 1, tx0:tx1 + 1] >= 1).all())
            skip[by, bx] = window_sky and bool(settled[by:by + 3, bx:bx + 3].all())
    return skip


def test_settled_sky_leaves_alone_exactly_the_blocks_the_rule_names(built):
    """After a still stretch: the words of frame f, then frame f + 1, its run words and its words.  The numpy restatement of the rule
    predicts the `left alone` bits of frame f + 1 exactly, and every block left alone is marked settled under the same epoch."""
    a, b = _pair()
    b.OnDestroy()
    try:
        for k in range(STILL):
            a.OnUpdate(); a.OnRender()
        ctx = a.context
        before, epoch = ctx.settled_words()
        parity = ctx.frame_parity()
        a.OnUpdate(); a.OnRender()
        runs, _ = ctx.sky_runs()
        after, epoch_after = ctx.settled_words()
        assert epoch_after == epoch and ctx.frame_parity() == parity ^ 1
        assert before.shape == (2, (H + 3) // 4, (W + 63) // 64) and runs.shape == ((H + 15) // 16, (W + 15) // 16)
        want = _rule(runs, before[parity], epoch)
        now = after[parity ^ 1]
        assert ((now >> 8) == epoch).all()
        got = (now & SKIPPED) != 0
        print("blocks %d, window over sky and settled with their neighbours %d, left alone %d" % (want.size, int(want.sum()), int(got.sum())))
        np.testing.assert_array_equal(got, want)
        assert int(want.sum()) > 0
        assert ((now[got] & SETTLED) != 0).all()
    finally:
        a.OnDestroy()
