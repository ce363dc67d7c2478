"""Recursion depth on the GPU (rtggx_set_max_recursion_depth, -recursion N; include/rtggx.h, DESIGN.md "Recursion depth").  Its parity
status: depth 1 pinned to the oracle (the rest of the suite); depths 2..4 have no counterpart in the reference and are pinned bit for bit to
the CPU restatement (tests/recursion_ref.cpp), which reproduces the oracle at depth 1 (tests/test_recursion_host.py); the denoiser pinned to
the oracle's when the oracle is given the restatement's raw images."""
import numpy as np
import pytest

import assets
import gpu_support as G
from gpu_support import check_raw
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FRAME_WORDS = G.GBUFFER_MIN + G.RAW      # the frame's own words: what a strip, or a context with another history, shares with its twin
IMAGES = FRAME_WORDS + G.DENOISED


def set_depth(p, depth):
    p.ctx.set_max_recursion_depth(depth); p.o.set_max_recursion_depth(depth)


@pytest.mark.parametrize("vndf", [False, True], ids=["ndf", "vndf"])
@pytest.mark.parametrize("metallic", [(1.0, 1.0), (0.25, 0.5), (1.0, 0.75)], ids=["metal", "diffuse", "metal-ground"])
@pytest.mark.parametrize("mesh", ["bunny.obj", "dragon.obj"], ids=["bunny", "dragon"])
def test_depth_2_and_3_equal_the_restatement(built, mesh, metallic, vndf):
    """Three frames at depth 2, then three at depth 3, on one context: raw images and G-buffer bit-exact, the ray count equal, the denoised
    HDR within 1e-3 of the oracle's denoiser fed the restatement's raw images (test_gpu_parity's check_frame)."""
    p = G.restated_pair(320, 180, depth=2, entry="depth", mesh=mesh, metallic=metallic, vndf=vndf)
    try:
        rays = {}
        for depth in (2, 3):
            set_depth(p, depth)
            for f in range(3):
                p.frame(); p.check_frame("%s depth %d frame %d" % (mesh, depth, f))
            rays[depth] = p.rays
        assert rays[3] > rays[2] > 0
    finally:
        p.close()


def test_full_size_frame_at_depth_2(built):
    p = G.restated_pair(1920, 1080, depth=2, entry="depth")
    try:
        p.frame(); check_raw(p, "1080p bunny depth 2")
    finally:
        p.close()


def test_depth_4_and_back_to_1(built):
    """Depth 4 against the restatement, then depth 3 and back to 1: a context that went to depth 3 and returned renders the frames of one
    that never left depth 1 (raw images bit-identical, and the ray count), and depth 1 is the oracle's."""
    p = G.restated_pair(320, 180, depth=4, entry="depth", metallic=(0.25, 0.5))
    b = G.app(320, 180, ["-metallic", 0.25, 0.5])
    try:
        p.frame(); check_raw(p, "depth 4")
        b.OnUpdate(); b.OnRender()
        set_depth(p, 3)
        for f in range(2):
            p.frame(); check_raw(p, "depth 3 frame %d" % f)
            b.OnUpdate(); b.OnRender()
        set_depth(p, 1)
        for f in range(3):
            p.frame(); check_raw(p, "back at depth 1, frame %d" % f)
            b.OnUpdate(); b.OnRender()
            G.assert_same(G.images(p.app, FRAME_WORDS), G.images(b, FRAME_WORDS), "back at depth 1, frame %d" % f)
            assert p.ctx.ray_count() == b.context.ray_count()
        # the oracle's own depth-1 renderer on the same frame
        p.o.ray_trace_depth1_oracle()
        for gid, oid in ((p.capi.BUF_RT_REFL, O.BUF_RT_REFL), (p.capi.BUF_RT_DIFF, O.BUF_RT_DIFF)):
            np.testing.assert_array_equal(p.ctx.readback(gid), p.o.buffer(oid))
    finally:
        p.close(); b.OnDestroy()


@pytest.mark.parametrize("W,H,force_small", [(640, 360, 0), (640, 360, 1), (1920, 1080, -1)], ids=["640x360-full-size-placement", "640x360-small-placement", "1080p"])
def test_free_running_frames_equal_synchronised_ones(built, W, H, force_small):
    extra = ["-recursion", 2, "-metallic", 1.0, 0.5]
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
            assert a.context.placement(1)[1]["shade"] == "B", "small launches shade (and trace the later levels) on the traversal's stream"
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_async_compute_off_and_caller_owned_stream_change_nothing(built):
    import torch
    extra = ["-recursion", 2, "-metallic", 1.0, 0.5]
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


def test_quarter_rate_at_depth_2(built):
    """Rate 4 at depth 2: traced pixels equal the full-rate depth-2 frame (the restatement), the reconstructed ones their restatement."""
    p = G.restated_pair(640, 360, depth=2, entry="depth", metallic=(1.0, 0.5))
    try:
        p.ctx.set_ray_rate(4)
        prev = None
        for f in range(4):
            full = G.quad_frame(p)
            prev = G.check_quad_frame(p, full, "rate 4 depth 2 frame %d" % f, prev)
    finally:
        p.close()


def test_strip_rows_equal_the_full_frame(built):
    a, b = G.app(640, 360, ["-recursion", 3, "-metallic", 0.25, 0.5]), G.app(640, 360, ["-recursion", 3, "-metallic", 0.25, 0.5])
    try:
        b.context.set_strip(100, 260)
        for f in range(3):
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            ia, ib = G.images(a, FRAME_WORDS), G.images(b, FRAME_WORDS)
            for k in ia:
                np.testing.assert_array_equal(ia[k][100:260], ib[k][100:260], err_msg="frame %d: %s" % (f, k))
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_strips_through_rccl_at_depth_2(built):
    G.strips_through_rccl_equal_the_full_frame(480, 272, 2, False, 3, extra=("-recursion", "2"))


def test_deforming_mesh_at_depth_2(built):
    """One frame of a refitted (deformed) model at depth 2 against the restatement given the refitted tree."""
    p = G.restated_pair(320, 180, depth=2, entry="depth", metallic=(1.0, 0.5))
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


def test_refusals_leave_the_depth_unchanged(built):
    from raytracedggx_amd import capi
    c = capi.Context(64, 64)
    try:
        for bad in (0, 5, 100, 2 ** 32 - 1):
            with pytest.raises(capi.RtggxError, match="rtggx_set_max_recursion_depth"):
                c.set_max_recursion_depth(bad)
        for good in (1, 2, 3, 4, 1):
            c.set_max_recursion_depth(good)
    finally:
        c.close()
    a, b = G.app(320, 180, ["-recursion", 2, "-metallic", 1.0, 0.5]), G.app(320, 180, ["-recursion", 2, "-metallic", 1.0, 0.5])
    try:
        for f in range(2):
            for bad in (0, 5):
                with pytest.raises(capi.RtggxError):
                    a.context.set_max_recursion_depth(bad)
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
            assert a.context.ray_count() == b.context.ray_count()
    finally:
        a.OnDestroy(); b.OnDestroy()
