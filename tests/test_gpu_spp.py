"""Samples per pixel on the GPU (rtggx_set_samples_per_pixel, -spp N; include/rtggx.h, DESIGN.md "Samples per pixel").  Its parity status:
N = 1 pinned to the oracle (the rest of the suite); N = 2, 4, 8 have no counterpart in the reference and are pinned bit for bit to the CPU
restatement (tests/spp_ref.cpp), which reproduces the oracle at N = 1 (tests/test_spp_host.py); the denoiser pinned to the oracle's when
the oracle is given the restatement's raw images.  Every pixel of every frame is compared."""
import numpy as np
import pytest

import assets
import gpu_support as G
from gpu_support import check_raw
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FRAME_WORDS = G.GBUFFER_MIN + G.RAW      # the frame's own words: what a strip, or a context with another history, shares with its twin
IMAGES = FRAME_WORDS + G.DENOISED


def set_samples(p, samples):
    p.ctx.set_samples_per_pixel(samples); p.o.set_samples_per_pixel(samples)


@pytest.mark.parametrize("vndf", [False, True], ids=["ndf", "vndf"])
@pytest.mark.parametrize("metallic", [(1.0, 1.0), (0.25, 0.5), (1.0, 0.75)], ids=["metal", "diffuse", "metal-ground"])
@pytest.mark.parametrize("mesh,samples", [("bunny.obj", 2), ("bunny.obj", 4), ("bunny.obj", 8), ("dragon.obj", 4)], ids=["bunny-2", "bunny-4", "bunny-8", "dragon-4"])
def test_raw_frames_equal_the_restatement(built, mesh, samples, metallic, vndf):
    """Three frames at 320x180: raw images and G-buffer bit-exact, the ray count equal, the denoised HDR within check_frame's bars of the
    oracle's denoiser fed the restatement's raw images."""
    p = G.restated_pair(320, 180, samples=samples, entry="spp", mesh=mesh, metallic=metallic, vndf=vndf)
    try:
        for f in range(3):
            p.frame(); p.check_frame("%s N = %d frame %d" % (mesh, samples, f))
        assert p.rays > 0
    finally:
        p.close()


def test_full_size_frame_at_2_samples(built):
    p = G.restated_pair(1920, 1080, samples=2, entry="spp")
    try:
        p.frame(); check_raw(p, "1080p bunny N = 2")
    finally:
        p.close()


@pytest.mark.parametrize("samples,depth", [(2, 2), (4, 3)], ids=["2x-depth2", "4x-depth3"])
def test_samples_times_depth(built, samples, depth):
    p = G.restated_pair(320, 180, samples=samples, entry="spp", depth=depth, metallic=(0.25, 0.5))
    try:
        for f in range(2):
            p.frame(); check_raw(p, "N = %d depth %d frame %d" % (samples, depth, f))
    finally:
        p.close()


def test_8_samples_then_2_and_back_to_1(built):
    """N = 8 against the restatement, then 2, then back to 1, every frame raw and denoised (check_frame: the oracle's denoiser has seen the
    same history): a context that went to 8 and returned renders the raw frames and the ray counts of one that never left 1, and those are the oracle's."""
    p = G.restated_pair(320, 180, samples=8, entry="spp", metallic=(0.25, 0.5))
    b = G.app(320, 180, ["-metallic", 0.25, 0.5])
    try:
        p.frame(); p.check_frame("N = 8")
        b.OnUpdate(); b.OnRender()
        set_samples(p, 2)
        for f in range(2):
            p.frame(); p.check_frame("N = 2 frame %d" % f)
            b.OnUpdate(); b.OnRender()
        set_samples(p, 1)
        for f in range(3):
            p.frame(); p.check_frame("back at N = 1, frame %d" % f)
            b.OnUpdate(); b.OnRender()
            G.assert_same(G.images(p.app, FRAME_WORDS), G.images(b, FRAME_WORDS), "back at N = 1, frame %d" % f)
            assert p.ctx.ray_count() == b.context.ray_count()
        # the oracle's own one-sample renderer on the same frame
        p.o.ray_trace_oracle()
        for gid, oid in ((p.capi.BUF_RT_REFL, O.BUF_RT_REFL), (p.capi.BUF_RT_DIFF, O.BUF_RT_DIFF)):
            np.testing.assert_array_equal(p.ctx.readback(gid), p.o.buffer(oid))
    finally:
        p.close(); b.OnDestroy()


def test_a_context_that_never_left_1_after_a_round_trip_of_the_setting(built):
    """rtggx_set_samples_per_pixel(8) and (2) that never reach a frame -- the setting is taken over by rtggx_render_visibility -- and back to 1:
    every frame is the frame of a context that never heard of it: raw, denoised, back buffer, ray count."""
    a, b = G.app(320, 180, ["-metallic", 0.25, 0.5]), G.app(320, 180, ["-metallic", 0.25, 0.5])
    try:
        for f in range(4):
            a.context.set_samples_per_pixel(8); a.context.set_samples_per_pixel(2); a.context.set_samples_per_pixel(1)
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
            assert a.context.ray_count() == b.context.ray_count()
    finally:
        a.OnDestroy(); b.OnDestroy()


@pytest.mark.parametrize("W,H,force_small", [(640, 360, 0), (640, 360, 1), (1920, 1080, -1)], ids=["640x360-full-size-placement", "640x360-small-placement", "1080p"])
def test_free_running_frames_equal_synchronised_ones(built, W, H, force_small):
    extra = ["-spp", 2, "-metallic", 1.0, 0.5]
    a, b = G.app(W, H, extra), G.app(W, H, extra)
    try:
        for x in (a, b):
            x.context.placement(force_small)
        for f in range(16):
            a.OnUpdate(); a.OnRender(); a.context.sync()
            b.OnUpdate(); b.OnRender()
        G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "%dx%d placement %d after 16 frames" % (W, H, force_small))
        assert a.context.ray_count() == b.context.ray_count()
        if force_small == 1:
            assert a.context.placement(1)[1]["shade"] == "B", "small launches shade (and trace the later samples) on the traversal's stream"
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_async_compute_off_and_caller_owned_stream_change_nothing(built):
    import torch
    extra = ["-spp", 4, "-metallic", 1.0, 0.5]
    a, b, c = G.app(640, 360, extra), G.app(640, 360, extra + ["-sync"]), G.app(640, 360, extra)
    stream = torch.cuda.Stream()
    try:
        c.context.set_stream(stream.cuda_stream)
        for f in range(8):
            for x in (a, b, c):
                x.OnUpdate(); x.OnRender()
        torch.cuda.synchronize()
        ia = G.images(a, IMAGES)
        G.assert_same(ia, G.images(b, IMAGES), "async compute off")
        G.assert_same(ia, G.images(c, IMAGES), "caller-owned stream")
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


def test_tile_words_off_and_still_sky_off_change_nothing(built):
    extra = ["-spp", 4, "-metallic", 1.0, 0.5]
    a, b, c = G.app(640, 360, extra), G.app(640, 360, extra), G.app(640, 360, extra)
    try:
        b.context.tile_words(False)
        c.context.static_sky(False)
        for f in range(12):      # (beyond the still-sky threshold: a's sky tiles are being left alone)
            for x in (a, b, c):
                x.OnUpdate(); x.OnRender()
        ia = G.images(a, IMAGES)
        G.assert_same(ia, G.images(b, IMAGES), "tile words off")
        G.assert_same(ia, G.images(c, IMAGES), "still sky off")
        assert a.context.ray_count() == b.context.ray_count() == c.context.ray_count()
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


def test_strip_rows_equal_the_full_frame(built):
    a, b = G.app(640, 360, ["-spp", 4, "-metallic", 0.25, 0.5]), G.app(640, 360, ["-spp", 4, "-metallic", 0.25, 0.5])
    try:
        b.context.set_strip(100, 260)
        for f in range(3):
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            ia, ib = G.images(a, FRAME_WORDS), G.images(b, FRAME_WORDS)
            for k in ia:
                np.testing.assert_array_equal(ia[k][100:260], ib[k][100:260], err_msg="frame %d: %s" % (f, k))
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_strips_through_rccl_at_2_samples(built):
    G.strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=("-spp", "2"))


def test_deforming_mesh_at_2_samples(built):
    """One frame of a refitted (deformed) model at N = 2 against the restatement given the refitted tree."""
    p = G.restated_pair(320, 180, samples=2, entry="spp", metallic=(1.0, 0.5))
    try:
        p.frame(); check_raw(p, "before the deformation")
        v0, idx, _ = O.obj_import(assets.path("bunny.obj"))
        v = G.wave(v0, 1)
        p.ctx.refit_as(1, v)
        p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
        p.o.set_mesh(1, v, idx)
        p.give_oracle_the_device_trees(refitted=True)
        p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
        p.o.update_as(); p.o.render_visibility(); p.rays = p.o.ray_trace()
        check_raw(p, "deformed")
        assert p.ctx.placement()[0]["deforming"]
    finally:
        p.close()


def test_refusals_leave_the_context_unchanged(built):
    from raytracedggx_amd import capi
    c = capi.Context(64, 64)
    try:
        for bad in (0, 3, 5, 6, 7, 9, 16, 2 ** 32 - 1):
            with pytest.raises(capi.RtggxError, match="rtggx_set_samples_per_pixel"):
                c.set_samples_per_pixel(bad)
        for good in (1, 2, 4, 8, 1):
            c.set_samples_per_pixel(good)
        c.set_ray_rate(4)
        with pytest.raises(capi.RtggxError, match="rtggx_set_samples_per_pixel"):
            c.set_samples_per_pixel(2)
        c.set_samples_per_pixel(1)
        c.set_ray_rate(1)
        c.set_samples_per_pixel(2)
        with pytest.raises(capi.RtggxError, match="rtggx_set_ray_rate"):
            c.set_ray_rate(4)
    finally:
        c.close()
    extra = ["-spp", 2, "-metallic", 1.0, 0.5]
    a, b = G.app(320, 180, extra), G.app(320, 180, extra)
    try:
        for f in range(3):
            for bad in (0, 3, 16):
                with pytest.raises(capi.RtggxError):
                    a.context.set_samples_per_pixel(bad)
            with pytest.raises(capi.RtggxError):
                a.context.set_ray_rate(4)
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
            assert a.context.ray_count() == b.context.ray_count()
    finally:
        a.OnDestroy(); b.OnDestroy()
    # the other order: a rate-4 context refuses N > 1 and keeps rendering rate-4 frames
    a, b = G.app(320, 180, ["-rayrate", 4]), G.app(320, 180, ["-rayrate", 4])
    try:
        for f in range(3):
            with pytest.raises(capi.RtggxError):
                a.context.set_samples_per_pixel(4)
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "rate 4 frame %d" % f)
            assert a.context.ray_count() == b.context.ray_count()
    finally:
        a.OnDestroy(); b.OnDestroy()
