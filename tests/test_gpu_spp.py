"""Samples per pixel on the GPU (rtggx_set_samples_per_pixel, -spp N; include/rtggx.h, DESIGN.md "Samples per pixel").  Its parity status:
N = 1 pinned to the oracle (the rest of the suite); N = 2, 4, 8 have no counterpart in the reference and are pinned bit for bit to the CPU
restatement (tests/spp_ref.cpp), which reproduces the oracle at N = 1 (tests/test_spp_host.py); the denoiser pinned to the oracle's when
the oracle is given the restatement's raw images.  Every pixel of every frame is compared."""
import numpy as np
import pytest

import assets
import spp_ref as SR
import test_gpu_parity as GP
import test_gpu_ray_rate as QR
from oracle import oracle as O
from test_gpu_parity import Pair

pytestmark = pytest.mark.gpu


def spp_pair(W, H, samples, depth=1, mesh="bunny.obj", metallic=None, vndf=False):
    """test_gpu_parity.Pair with the restatement as its oracle, both at `samples` and `depth`."""
    orig = GP.O.Oracle
    GP.O.Oracle = lambda w, h: SR.Oracle(w, h, depth=depth, samples=samples)
    try:
        p = Pair(W, H, mesh=mesh, metallic=metallic)
    finally:
        GP.O.Oracle = orig
    p.ctx.set_samples_per_pixel(samples)
    if depth != 1:
        p.ctx.set_max_recursion_depth(depth)
    if vndf:
        p.ctx.set_sampler(True); p.o.set_sampler(True)
    return p


def set_samples(p, samples):
    p.ctx.set_samples_per_pixel(samples); p.o.set_samples_per_pixel(samples)


def check_raw(p, label):
    """G-buffer words, RayTracingOut0/1 and the ray count: bit for bit / equal."""
    capi, ctx, o = p.capi, p.ctx, p.o
    for name, gid, oid in (("visibility", capi.BUF_VISIBILITY, O.BUF_VISIBILITY), ("depth", capi.BUF_DEPTH, O.BUF_DEPTH),
                           ("normal", capi.BUF_NORMAL, O.BUF_NORMAL), ("roughMetal", capi.BUF_ROUGH_METAL, O.BUF_ROUGH_METAL),
                           ("velocity", capi.BUF_VELOCITY, O.BUF_VELOCITY), ("rt_refl", capi.BUF_RT_REFL, O.BUF_RT_REFL),
                           ("rt_diff", capi.BUF_RT_DIFF, O.BUF_RT_DIFF)):
        np.testing.assert_array_equal(ctx.readback(gid), o.buffer(oid), err_msg="%s: %s not bit-exact" % (label, name))
    assert ctx.ray_count() == p.rays, "%s: ray count %d, restatement %d" % (label, ctx.ray_count(), p.rays)


def _images(app, with_denoised=True):
    from raytracedggx_amd import capi
    ctx = app.context
    ctx.sync()
    ids = [("vis", capi.BUF_VISIBILITY), ("normal", capi.BUF_NORMAL), ("rm", capi.BUF_ROUGH_METAL), ("refl", capi.BUF_RT_REFL), ("diff", capi.BUF_RT_DIFF)]
    if with_denoised:
        ids += [("flt_rfl", capi.BUF_FLT_RFL), ("flt_dff", capi.BUF_FLT_DFF), ("tss0", capi.BUF_TSS0), ("tss1", capi.BUF_TSS0 + 1), ("back", capi.BUF_BACKBUFFER)]
    return {n: ctx.readback(b) for n, b in ids}


def _assert_same(a, b, label):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s differs" % (label, k))


def _app(W, H, extra=(), mesh="bunny.obj"):
    from raytracedggx_amd import app
    return app.RayTracedGGX(["-mesh", assets.path(mesh), "-env", assets.path("rnl_cross.dds"), "-width", W, "-height", H] + list(extra))


@pytest.mark.parametrize("vndf", [False, True], ids=["ndf", "vndf"])
@pytest.mark.parametrize("metallic", [(1.0, 1.0), (0.25, 0.5), (1.0, 0.75)], ids=["metal", "diffuse", "metal-ground"])
@pytest.mark.parametrize("mesh,samples", [("bunny.obj", 2), ("bunny.obj", 4), ("bunny.obj", 8), ("dragon.obj", 4)], ids=["bunny-2", "bunny-4", "bunny-8", "dragon-4"])
def test_raw_frames_equal_the_restatement(built, mesh, samples, metallic, vndf):
    """Three frames at 320x180: raw images and G-buffer bit-exact, the ray count equal, the denoised HDR within check_frame's bars of the
    oracle's denoiser fed the restatement's raw images."""
    p = spp_pair(320, 180, samples, mesh=mesh, metallic=metallic, vndf=vndf)
    try:
        for f in range(3):
            p.frame(); p.check_frame("%s N = %d frame %d" % (mesh, samples, f))
        assert p.rays > 0
    finally:
        p.close()


def test_full_size_frame_at_2_samples(built):
    p = spp_pair(1920, 1080, 2)
    try:
        p.frame(); check_raw(p, "1080p bunny N = 2")
    finally:
        p.close()


@pytest.mark.parametrize("samples,depth", [(2, 2), (4, 3)], ids=["2x-depth2", "4x-depth3"])
def test_samples_times_depth(built, samples, depth):
    p = spp_pair(320, 180, samples, depth=depth, metallic=(0.25, 0.5))
    try:
        for f in range(2):
            p.frame(); check_raw(p, "N = %d depth %d frame %d" % (samples, depth, f))
    finally:
        p.close()


def test_8_samples_then_2_and_back_to_1(built):
    """N = 8 against the restatement, then 2, then back to 1, every frame raw and denoised (check_frame: the oracle's denoiser has seen the
    same history): a context that went to 8 and returned renders the raw frames and the ray counts of one that never left 1, and those are the oracle's."""
    p = spp_pair(320, 180, 8, metallic=(0.25, 0.5))
    b = _app(320, 180, ["-metallic", 0.25, 0.5])
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
            _assert_same(_images(p.app, with_denoised=False), _images(b, with_denoised=False), "back at N = 1, frame %d" % f)
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
    a, b = _app(320, 180, ["-metallic", 0.25, 0.5]), _app(320, 180, ["-metallic", 0.25, 0.5])
    try:
        for f in range(4):
            a.context.set_samples_per_pixel(8); a.context.set_samples_per_pixel(2); a.context.set_samples_per_pixel(1)
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            _assert_same(_images(a), _images(b), "frame %d" % f)
            assert a.context.ray_count() == b.context.ray_count()
    finally:
        a.OnDestroy(); b.OnDestroy()


@pytest.mark.parametrize("W,H,force_small", [(640, 360, 0), (640, 360, 1), (1920, 1080, -1)], ids=["640x360-full-size-placement", "640x360-small-placement", "1080p"])
def test_free_running_frames_equal_synchronised_ones(built, W, H, force_small):
    extra = ["-spp", 2, "-metallic", 1.0, 0.5]
    a, b = _app(W, H, extra), _app(W, H, extra)
    try:
        for x in (a, b):
            x.context.placement(force_small)
        for f in range(16):
            a.OnUpdate(); a.OnRender(); a.context.sync()
            b.OnUpdate(); b.OnRender()
        _assert_same(_images(a), _images(b), "%dx%d placement %d after 16 frames" % (W, H, force_small))
        assert a.context.ray_count() == b.context.ray_count()
        if force_small == 1:
            assert a.context.placement(1)[1]["shade"] == "B", "small launches shade (and trace the later samples) on the traversal's stream"
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_async_compute_off_and_caller_owned_stream_change_nothing(built):
    import torch
    extra = ["-spp", 4, "-metallic", 1.0, 0.5]
    a, b, c = _app(640, 360, extra), _app(640, 360, extra + ["-sync"]), _app(640, 360, extra)
    stream = torch.cuda.Stream()
    try:
        c.context.set_stream(stream.cuda_stream)
        for f in range(8):
            for x in (a, b, c):
                x.OnUpdate(); x.OnRender()
        torch.cuda.synchronize()
        ia = _images(a)
        _assert_same(ia, _images(b), "async compute off")
        _assert_same(ia, _images(c), "caller-owned stream")
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


def test_tile_words_off_and_still_sky_off_change_nothing(built):
    extra = ["-spp", 4, "-metallic", 1.0, 0.5]
    a, b, c = _app(640, 360, extra), _app(640, 360, extra), _app(640, 360, extra)
    try:
        b.context.tile_words(False)
        c.context.static_sky(False)
        for f in range(12):      # (beyond the still-sky threshold: a's sky tiles are being left alone)
            for x in (a, b, c):
                x.OnUpdate(); x.OnRender()
        ia = _images(a)
        _assert_same(ia, _images(b), "tile words off")
        _assert_same(ia, _images(c), "still sky off")
        assert a.context.ray_count() == b.context.ray_count() == c.context.ray_count()
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


def test_strip_rows_equal_the_full_frame(built):
    a, b = _app(640, 360, ["-spp", 4, "-metallic", 0.25, 0.5]), _app(640, 360, ["-spp", 4, "-metallic", 0.25, 0.5])
    try:
        b.context.set_strip(100, 260)
        for f in range(3):
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            ia, ib = _images(a, with_denoised=False), _images(b, with_denoised=False)
            for k in ia:
                np.testing.assert_array_equal(ia[k][100:260], ib[k][100:260], err_msg="frame %d: %s" % (f, k))
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_strips_through_rccl_at_2_samples(built):
    GP._strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=("-spp", "2"))


def test_deforming_mesh_at_2_samples(built):
    """One frame of a refitted (deformed) model at N = 2 against the restatement given the refitted tree."""
    p = spp_pair(320, 180, 2, metallic=(1.0, 0.5))
    try:
        p.frame(); check_raw(p, "before the deformation")
        v0, idx, _ = O.obj_import(assets.path("bunny.obj"))
        v = GP._wave(v0, 1)
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
    capi = QR.ctx_capi()
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
    a, b = _app(320, 180, extra), _app(320, 180, extra)
    try:
        for f in range(3):
            for bad in (0, 3, 16):
                with pytest.raises(capi.RtggxError):
                    a.context.set_samples_per_pixel(bad)
            with pytest.raises(capi.RtggxError):
                a.context.set_ray_rate(4)
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            _assert_same(_images(a), _images(b), "frame %d" % f)
            assert a.context.ray_count() == b.context.ray_count()
    finally:
        a.OnDestroy(); b.OnDestroy()
    # the other order: a rate-4 context refuses N > 1 and keeps rendering rate-4 frames
    a, b = _app(320, 180, ["-rayrate", 4]), _app(320, 180, ["-rayrate", 4])
    try:
        for f in range(3):
            with pytest.raises(capi.RtggxError):
                a.context.set_samples_per_pixel(4)
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            _assert_same(_images(a), _images(b), "rate 4 frame %d" % f)
            assert a.context.ray_count() == b.context.ray_count()
    finally:
        a.OnDestroy(); b.OnDestroy()
