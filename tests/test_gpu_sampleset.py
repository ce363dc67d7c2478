"""The sample-set size on the GPU (rtggx_set_sample_set, -sampleset M; include/rtggx.h, DESIGN.md "Sample-set size").  Its parity status:
M = 256 is the reference's renderer, pinned to the oracle by the rest of the suite; M = 512 .. 65536 have no counterpart in the reference
and are pinned bit for bit to the CPU restatement (tests/sampleset_ref.cpp), which reproduces tests/spp_ref.cpp -- and through it the
oracle -- at M = 256 (tests/test_sampleset_host.py).  Every pixel of every frame is compared.  The small frame is 100x54: the width no
multiple of 16, the height no multiple of 16, 28 workgroups of ray generation."""
import numpy as np
import pytest

import accum_ref as AR
import gpu_support as G
import ray_rate_ref as R
from gpu_support import FRAME_INDEX_OFFSET

pytestmark = pytest.mark.gpu

W, H = 100, 54
FRAME_WORDS = G.GBUFFER + G.RAW + G.RAYS
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS


def frame_at_index(p, index):
    """One frame of the pair with FrameIndex patched into the host layer's constants: the product through the C ABI, the restatement's."""
    p.app.OnUpdate()
    k = p.app.frame_constants().copy()
    k[FRAME_INDEX_OFFSET:FRAME_INDEX_OFFSET + 4] = np.array([index], np.uint32).view(np.uint8)
    c = p.ctx
    c.update_frame(k); c.update_as(); c.render_visibility(); c.ray_trace(); c.denoise(); c.tone_map(); c.sync()
    p.o.set_frame_constants(k.tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
    p.o.update_as(); p.o.render_visibility(); p.rays = p.o.ray_trace()


# ---- 1. raw frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_set", [1024, 65536])
@pytest.mark.parametrize("vndf", [False, True], ids=["ndf", "vndf"])
@pytest.mark.parametrize("metallic", [(1.0, 1.0), (0.25, 0.5), (1.0, 0.75)], ids=["metal", "diffuse", "metal-ground"])
def test_raw_frames_equal_the_restatement(built, metallic, vndf, sample_set):
    """Bunny at 100x54, FrameIndex 0, 255, 256 and M - 1 patched into the constants: G-buffer, both raw images and the ray count.  At
    M = 1024 three quarters of the pixels draw a slot beyond the 256-entry table, at 65536 all but 0.4 %."""
    p = G.restated_pair(W, H, sample_set=sample_set, entry="sampleset", metallic=metallic, vndf=vndf)
    try:
        for index in (0, 255, 256, sample_set - 1):
            frame_at_index(p, index)
            G.check_raw(p, "M = %d index %d" % (sample_set, index), require_rays=True)
    finally:
        p.close()


# ---- 2. combinations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,samples,depth,vndf,metallic", [("bunny.obj", 4, 2, True, (0.25, 0.5)), ("bunny.obj", 8, 1, False, None), ("dragon.obj", 2, 1, False, None)],
                         ids=["spp4-depth2-vndf-diffuse", "spp8", "dragon-spp2"])
def test_samples_and_depth_at_4096(built, mesh, samples, depth, vndf, metallic):
    p = G.restated_pair(W, H, sample_set=4096, entry="sampleset", samples=samples, depth=depth, mesh=mesh, metallic=metallic, vndf=vndf)
    try:
        for f in range(2):
            p.frame(); G.check_raw(p, "%s M = 4096 N = %d depth %d frame %d" % (mesh, samples, depth, f), require_rays=True)
    finally:
        p.close()


def test_quarter_rate_at_4096_traces_the_full_rate_twins_pixels(built):
    """-rayrate 4 at M = 4096: the traced pixels' words are those of a rate-1 twin at the same M, the G-buffer is the twin's everywhere, and
    the rays are those of the traced covered pixels (one each: all metal)."""
    from raytracedggx_amd import capi
    a, b = G.app(W, H, ["-sampleset", 4096, "-rayrate", 4]), G.app(W, H, ["-sampleset", 4096])
    try:
        for f in range(5):      # (every phase of FrameIndex & 3, and the first again)
            G.frame(a); G.frame(b)
            ia, ib = G.images(a, FRAME_WORDS), G.images(b, FRAME_WORDS)
            for k in ("vis", "depth", "normal", "rm", "velocity"):
                np.testing.assert_array_equal(ia[k], ib[k], err_msg="frame %d: %s" % (f, k))
            assert G.frame_index(a) == G.frame_index(b) == f
            traced = R.traced_mask(W, H, f)
            covered = ia["vis"] != 0
            at = traced | ~covered
            np.testing.assert_array_equal(ia["refl"][at], ib["refl"][at], err_msg="frame %d: RayTracingOut0 at traced / background pixels" % f)
            # a reflection ray per covered pixel whose NoL > 0 (a word of 0 where it is not: include/rtggx.h) -- of the traced ones only
            assert int(ia["rays"][0]) <= int((traced & covered).sum()) and 0 < int(ia["rays"][0])
            assert 0.2 * int(ib["rays"][0]) <= int(ia["rays"][0]) <= 0.3 * int(ib["rays"][0])
        assert a.context.readback(capi.BUF_RT_REFL).any()
    finally:
        a.OnDestroy(); b.OnDestroy()


# ---- 3. the default is untouched -----------------------------------------------------------------------------------------------------
def test_setting_256_is_never_having_set_it(built):
    a, b = G.app(320, 180, ["-metallic", 0.25, 0.5]), G.app(320, 180, ["-metallic", 0.25, 0.5])
    try:
        a.context.set_sample_set(256)
        for f in range(6):
            if f == 3:
                a.context.set_sample_set(256)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_4096_and_back_renders_the_frames_of_a_twin_that_never_left(built):
    a, b = G.app(320, 180, ["-metallic", 0.25, 0.5]), G.app(320, 180, ["-metallic", 0.25, 0.5])
    try:
        G.frame(a); G.frame(b)
        a.context.set_sample_set(4096)
        differed = False
        for f in range(3):
            G.frame(a); G.frame(b)
            ia, ib = G.images(a, FRAME_WORDS), G.images(b, FRAME_WORDS)
            for k in ("vis", "depth", "normal", "rm", "velocity"):      # nothing else of a frame depends on M
                np.testing.assert_array_equal(ia[k], ib[k], err_msg="at 4096, frame %d: %s" % (f, k))
            differed = differed or not np.array_equal(ia["refl"], ib["refl"])
        assert differed, "the setting reached no frame"
        a.context.set_sample_set(256)
        for f in range(3):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, FRAME_WORDS), G.images(b, FRAME_WORDS), "back at 256, frame %d" % f)
    finally:
        a.OnDestroy(); b.OnDestroy()


# ---- 4. ordering ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["small", "full-size", "caller-stream"])
def test_free_running_frames_with_the_set_switched_equal_synchronised_ones(built, mode):
    """16 frames, M 256 -> 65536 in front of frame 5 -> 1024 in front of frame 10, one context synchronised after every frame, the other
    free-running: a frame in flight keeps its table and its mask."""
    import torch
    extra = ["-metallic", 1.0, 0.5]
    a, b = G.app(320, 180, extra), G.app(320, 180, extra)
    stream = torch.cuda.Stream() if mode == "caller-stream" else None
    try:
        for x in (a, b):
            if stream is not None:
                x.context.set_stream(stream.cuda_stream)
            else:
                x.context.placement(1 if mode == "small" else 0)
        for f in range(16):
            for x in (a, b):
                if f == 5:
                    x.context.set_sample_set(65536)
                if f == 10:
                    x.context.set_sample_set(1024)
                G.frame(x)
            a.context.sync()
            if f in (4, 9):
                G.assert_same(G.images(a, FRAME_WORDS), G.images(b, FRAME_WORDS), "%s: frame %d" % (mode, f))
        torch.cuda.synchronize()
        G.assert_same(G.images(a, FRAME_WORDS), G.images(b, FRAME_WORDS), "%s: after 16 frames" % mode)
    finally:
        a.OnDestroy(); b.OnDestroy()


# ---- 5. the host's counter -----------------------------------------------------------------------------------------------------------
def test_host_frame_counter_wraps_at_the_set_size(built):
    """Word 111 of the frame constants (FrameIndex) through app with -sampleset 1024 -dt 0 at 64x36: 256 after 257 frames, 1023 after 1024,
    0 after 1025; the default app reads 0 after 257."""
    a, b = G.app(64, 36, ["-sampleset", 1024, "-dt", 0]), G.app(64, 36, ["-dt", 0])
    try:
        seen = {}
        for f in range(1, 1026):
            G.frame(a)
            if f in (257, 1024, 1025):
                seen[f] = int(a.frame_constants().view(np.uint32)[111])
        assert seen == {257: 256, 1024: 1023, 1025: 0}
        for f in range(257):
            G.frame(b)
        assert int(b.frame_constants().view(np.uint32)[111]) == 0
        a.context.sync(); b.context.sync()
    finally:
        a.OnDestroy(); b.OnDestroy()


# ---- 6. strips -----------------------------------------------------------------------------------------------------------------------
def test_two_strips_at_1024_equal_the_whole_frame(built):
    extra = ["-sampleset", 1024, "-metallic", 0.25, 0.5]
    whole, top, bottom = G.app(W, H, extra), G.app(W, H, extra), G.app(W, H, extra)
    try:
        top.context.set_strip(0, 30); bottom.context.set_strip(30, H)
        for f in range(3):
            for x in (whole, top, bottom):
                G.frame(x)
            iw, it, ib = (G.images(x, FRAME_WORDS) for x in (whole, top, bottom))
            for k in ("vis", "normal", "rm", "velocity", "refl", "diff"):
                np.testing.assert_array_equal(it[k][:30], iw[k][:30], err_msg="frame %d: %s, rows 0..29" % (f, k))
                np.testing.assert_array_equal(ib[k][30:], iw[k][30:], err_msg="frame %d: %s, rows 30..53" % (f, k))
    finally:
        whole.OnDestroy(); top.OnDestroy(); bottom.OnDestroy()


# ---- 7. accumulation -----------------------------------------------------------------------------------------------------------------
def test_accumulation_at_4096_equals_its_restatement_and_survives_a_change_of_the_set(built):
    from raytracedggx_amd import capi
    metallic = (0.25, 0.5)
    a = G.app(W, H, ["-sampleset", 4096, "-metallic", metallic[0], metallic[1], "-accumulate", 64])
    try:
        acc = AR.Accumulator(H, W)

        def check(label):
            got = (a.context.readback(capi.BUF_ACC_REFL), a.context.readback(capi.BUF_ACC_DIFF), a.context.accumulated_frames())
            assert got[2] == acc.frames, label
            assert AR.same_bits(got[0], acc.refl).all() and AR.same_bits(got[1], acc.diff).all(), label

        for f in range(6):
            if f == 3:      # in mid-run: count and sums stay as they are (the reset is the caller's)
                a.context.set_sample_set(512)
                check("after set_sample_set")
            G.frame(a)
            c = a.context
            acc.add(c.readback(capi.BUF_RT_REFL), c.readback(capi.BUF_RT_DIFF), c.readback(capi.BUF_VISIBILITY), metallic)
            check("frame %d" % f)
        assert acc.frames == 6 and acc.refl.any() and acc.diff.any()
    finally:
        a.OnDestroy()


def test_accumulate_line_warns_past_m_frames_at_two_samples(built, tmp_path, capfd):
    """-spp 2 -accumulate through app at 64x36, M = 256: after 200 frames -- 400 samples, every index distinct -- the line states the set and
    does not warn; after 257 frames the first frame has come again and it does."""
    a = G.app(64, 36, ["-spp", 2, "-accumulate", 1000, "-dt", 0])
    try:
        for f in range(200):
            G.frame(a)
        capfd.readouterr()
        assert a.save_converged(str(tmp_path / "a.png"))
        out = capfd.readouterr().out
        assert "accumulated 200 frames" in out and "; sample set of 256" in out and "warning" not in out, out
        for f in range(57):
            G.frame(a)
        assert a.save_converged(str(tmp_path / "b.png"))
        out = capfd.readouterr().out
        assert "accumulated 257 frames" in out and "; sample set of 256\nwarning: 257 frames of 2 samples" in out and "repeat after 256 " in out, out
    finally:
        a.OnDestroy()


# ---- 8. still sky --------------------------------------------------------------------------------------------------------------------
def test_still_sky_with_the_set_changed_in_mid_run(built):
    """12 still frames at 320x180, M changed in front of frame 6, beside a twin with rtggx_debug_static_sky(0): every target of every frame.
    The change ends no run: the frame after it still leaves tiles alone (runs broken at frame 6 would stand at 2 there, below the
    threshold of RT_SETS + 2)."""
    from raytracedggx_amd import capi
    a, b = G.app(320, 180, ["-sharedmem"]), G.app(320, 180, ["-sharedmem"])
    targets = (capi.BUF_VISIBILITY, capi.BUF_DEPTH, capi.BUF_NORMAL, capi.BUF_ROUGH_METAL, capi.BUF_VELOCITY, capi.BUF_RT_REFL, capi.BUF_RT_DIFF,
               capi.BUF_FLT_RFL, capi.BUF_FLT_DFF, capi.BUF_TSS0, capi.BUF_TSS1, capi.BUF_BACKBUFFER)
    try:
        b.context.static_sky(False)
        for f in range(12):
            for x in (a, b):
                if f == 6:
                    x.context.set_sample_set(8192)
                G.frame(x)
            a.context.sync(); b.context.sync()
            for bid in targets:
                np.testing.assert_array_equal(a.context.readback(bid), b.context.readback(bid), err_msg="frame %d: buffer %d" % (f, bid))
            if f == 7:
                runs, threshold = a.context.sky_runs()
                assert int((runs >= threshold).sum()) > 0, "the change of the set ended the still-sky runs"
        runs, threshold = a.context.sky_runs()
        assert int((runs >= threshold).sum()) > 0
    finally:
        a.OnDestroy(); b.OnDestroy()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_unchanged(built):
    from raytracedggx_amd import capi
    c = capi.Context(64, 64)
    try:
        for bad in (0, 128, 255, 257, 3000, 131072):
            with pytest.raises(capi.RtggxError, match="rtggx_set_sample_set"):
                c.set_sample_set(bad)
        for good in (256, 512, 65536, 1024, 256):
            c.set_sample_set(good)
    finally:
        c.close()
    a, b = G.app(W, H, ["-sampleset", 2048]), G.app(W, H, ["-sampleset", 2048])
    try:
        for f in range(3):
            for bad in (0, 128, 255, 257, 3000, 131072):
                with pytest.raises(capi.RtggxError):
                    a.context.set_sample_set(bad)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
    finally:
        a.OnDestroy(); b.OnDestroy()
