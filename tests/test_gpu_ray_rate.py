"""Quarter-rate tracing on the GPU (rtggx_set_ray_rate(ctx, 4), -rayrate 4; DESIGN.md "Quarter-rate tracing").  Its parity status:
not pinned to the reference; pinned to the full-rate path (the CPU oracle) at the traced pixels and in the G-buffer; the reconstruction
pinned to its numpy restatement (tests/ray_rate_ref.py); the denoiser pinned to the oracle's when the oracle is given the same raw images."""
import numpy as np
import pytest

import gpu_support as G
import ray_rate_ref as R
from gpu_support import Pair, check_quad_frame, quad_frame, rel_l2
from oracle import oracle as O

pytestmark = pytest.mark.gpu

IMAGES = G.RAW + G.DENOISED      # what this module's twins are compared in


def ctx_capi():
    from raytracedggx_amd import capi
    return capi


def check_denoised(p, label):
    """The denoiser's outputs against the oracle's on the same raw images (test_gpu_parity's bars)."""
    capi, ctx, o = p.capi, p.ctx, p.o
    par = ctx.frame_parity()
    assert par == o.parity()
    for name, gid, oid in (("FilteredOut", capi.BUF_FLT_RFL, O.BUF_FLT_RFL), ("FilteredOut1", capi.BUF_FLT_DFF, O.BUF_FLT_DFF),
                           ("TemporalSSOut", capi.BUF_TSS0 + par, O.BUF_TSS0 + par)):
        g, r = O.unpack_rgba16f(ctx.readback(gid)), O.unpack_rgba16f(o.buffer(oid))
        fin = np.isfinite(r)
        np.testing.assert_array_equal(np.isfinite(g), fin, err_msg="%s: %s non-finite values differ from the oracle's" % (label, name))
        e = rel_l2(np.where(fin, g, 0.0), np.where(fin, r, 0.0))
        assert e < p.hdr_tol, "%s: %s relative L2 %.3e" % (label, name, e)
    g, r = O.unpack_rgba8(ctx.readback(capi.BUF_BACKBUFFER)).astype(int), O.unpack_rgba8(o.buffer(O.BUF_BACKBUFFER)).astype(int)
    assert np.abs(g - r).max() <= 1, "%s: back buffer" % label


def _quad_pair(W, H, metallic=None, shared_mem=False, vndf=False):
    p = Pair(W, H, metallic=metallic, shared_mem=shared_mem)
    if vndf:
        p.ctx.set_sampler(True); p.o.set_sampler(True)
    p.ctx.set_ray_rate(4)
    return p


@pytest.mark.parametrize("W,H,metallic,vndf", [(640, 360, None, False), (333, 187, None, False), (640, 360, (0.25, 0.5), False),
                                               (333, 187, (0.25, 0.5), False), (640, 360, (1.0, 0.5), True)],
                         ids=["640x360", "333x187", "640x360-diffuse", "333x187-diffuse", "640x360-metal-ground-vndf"])
def test_traced_pixels_equal_full_rate_and_reconstruction_its_restatement(built, W, H, metallic, vndf):
    p = _quad_pair(W, H, metallic, vndf=vndf)
    try:
        prev = None
        for f in range(6):      # every offset of the quad, and two frames that carry over from a rate-4 frame
            full = quad_frame(p)
            prev = check_quad_frame(p, full, "%dx%d frame %d" % (W, H, f), prev)
    finally:
        p.close()


@pytest.mark.parametrize("W,H,metallic,shared_mem", [(1920, 1080, None, False), (640, 360, (0.25, 0.5), True)], ids=["1080p", "640x360-sharedmem-diffuse"])
def test_denoise_chain_on_quarter_rate_input(built, W, H, metallic, shared_mem):
    p = _quad_pair(W, H, metallic, shared_mem=shared_mem)
    try:
        prev = None
        for f in range(3):
            full = quad_frame(p)
            prev = check_quad_frame(p, full, "%dx%d frame %d" % (W, H, f), prev)
            check_denoised(p, "%dx%d frame %d" % (W, H, f))
    finally:
        p.close()


@pytest.mark.parametrize("W,H", [(1920, 1080), (256, 144)], ids=["1080p", "256x144-small-launch"])
def test_free_running_frames_equal_synchronised_ones(built, W, H):
    extra = ["-rayrate", 4, "-metallic", 1.0, 0.5]
    a, b = G.app(W, H, extra), G.app(W, H, extra)
    try:
        for f in range(30):
            a.OnUpdate(); a.OnRender()
            b.OnUpdate(); b.OnRender(); b.context.sync()
        G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "%dx%d after 30 frames" % (W, H))
        if W == 256:
            assert a.context.placement()[0]["small"], "the small-launch placement"
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_async_compute_off_equals_on(built):
    extra = ["-rayrate", 4, "-metallic", 1.0, 0.5]
    a, b = G.app(640, 360, extra), G.app(640, 360, extra + ["-sync"])
    try:
        for f in range(8):
            a.OnUpdate(); a.OnRender(); b.OnUpdate(); b.OnRender()
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_deforming_mesh_at_rate_4_equals_rate_1_at_traced_pixels(built):
    capi = ctx_capi()
    extra = ["-deform", 0.3, "-metallic", 0.25, 0.5]
    a, b = G.app(640, 360, extra + ["-rayrate", 4]), G.app(640, 360, extra)
    try:
        for f in range(6):
            a.OnUpdate(); a.OnRender(); a.context.sync(); b.OnUpdate(); b.OnRender(); b.context.sync()
            ga, gb = G.gbuffer(a.context), G.gbuffer(b.context)
            for k in ga:
                np.testing.assert_array_equal(ga[k], gb[k], err_msg="frame %d: %s" % (f, k))
            traced = R.traced_mask(640, 360, G.frame_index(a)) | (ga["vis"] == 0)
            for bid in (capi.BUF_RT_REFL, capi.BUF_RT_DIFF):
                np.testing.assert_array_equal(a.context.readback(bid)[traced], b.context.readback(bid)[traced], err_msg="frame %d: buffer %d" % (f, bid))
    finally:
        a.OnDestroy(); b.OnDestroy()


@pytest.mark.parametrize("tile_words", [True, False], ids=["tile-words", "no-tile-words"])
def test_switching_rate_between_frames(built, tile_words):
    p = Pair(640, 360, metallic=(1.0, 0.5))
    try:
        p.ctx.tile_words(tile_words)
        prev = None
        for rate, frames in ((1, 2), (4, 5), (1, 3), (4, 2)):
            p.ctx.set_ray_rate(rate)
            for f in range(frames):
                label = "rate %d frame %d" % (rate, f)
                if rate == 1:
                    full = quad_frame(p, give_oracle_raw=False)
                    g = G.gbuffer(p.ctx)
                    for name, oid in (("vis", O.BUF_VISIBILITY), ("depth", O.BUF_DEPTH), ("normal", O.BUF_NORMAL), ("rm", O.BUF_ROUGH_METAL), ("velocity", O.BUF_VELOCITY)):
                        np.testing.assert_array_equal(g[name], p.o.buffer(oid), err_msg="%s: %s" % (label, name))
                    np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_REFL), full["refl"], err_msg=label)
                    np.testing.assert_array_equal(p.ctx.readback(p.capi.BUF_RT_DIFF), full["diff"], err_msg=label)
                    assert p.ctx.ray_count() == p.rays, label
                    prev = full["diff"]
                else:
                    full = quad_frame(p)
                    prev = check_quad_frame(p, full, label, prev)
    finally:
        p.close()


# Measured on an MI355X (bunny, 640x360, -dt 0, 32 frames): the rate-4 TemporalSSOut differs from the rate-1 one by 0.137 relative L2, while
# the rate-1 image itself moves by 0.014 between frames 28 and 32.  The difference is what the accumulated image keeps of the estimator,
# not drift: the bar sits 10 % above the measured value, so that a reconstruction that got worse fails here.
CONVERGENCE_BAR = 0.15


def test_static_scene_converges_towards_the_full_rate_image(built):
    capi = ctx_capi()
    a, b, v = G.app(640, 360, ["-dt", 0, "-rayrate", 4]), G.app(640, 360, ["-dt", 0]), G.app(640, 360, ["-dt", 0, "-vndf"])
    try:
        for f in range(32):
            for x in (a, b, v):
                x.OnUpdate(); x.OnRender()
            if f == 27:      # (for scale: how far the rate-1 image itself still moves in its last four frames)
                b.context.sync(); b28 = O.unpack_rgba16f(b.context.readback(capi.BUF_TSS0 + b.context.frame_parity())).astype(np.float64)
        tss = []
        for x in (a, b, v):
            x.context.sync()
            tss.append(O.unpack_rgba16f(x.context.readback(capi.BUF_TSS0 + x.context.frame_parity())).astype(np.float64))
        assert a.context.frame_parity() == b.context.frame_parity()

        def rel(p, q):
            fin = np.isfinite(p) & np.isfinite(q)
            return rel_l2(np.where(fin, p, 0.0), np.where(fin, q, 0.0))
        e = rel(tss[0], tss[1])
        # for scale: the rate-1 image against itself four frames earlier, and against another unbiased estimator at rate 1 (the VNDF sampler)
        print("rate 4 vs rate 1 TemporalSSOut after 32 static frames: relative L2 %.4f (rate 1, frame 28 vs 32: %.4f; rate 1 VNDF vs NDF: %.4f)" % (
            e, rel(b28, tss[1]), rel(tss[2], tss[1])))
        assert e < CONVERGENCE_BAR, "relative L2 %.4f" % e
    finally:
        a.OnDestroy(); b.OnDestroy(); v.OnDestroy()


def test_refusals(built):
    capi = ctx_capi()
    c = capi.Context(64, 64)
    try:
        for bad in (0, 2, 3, 8):
            with pytest.raises(capi.RtggxError, match="rtggx_set_ray_rate"):
                c.set_ray_rate(bad)
        c.set_strip(0, 32)
        with pytest.raises(capi.RtggxError, match="strip"):
            c.set_ray_rate(4)
        c.set_strip(0, 64)
        c.set_ray_rate(4)
        for rows in ((0, 32), (16, 64), (0, 0)):
            with pytest.raises(capi.RtggxError, match="rtggx_set_strip"):
                c.set_strip(*rows)
        c.set_strip(0, 64)
        c.set_ray_rate(1)
        c.set_strip(0, 32)
    finally:
        c.close()
    # rate 1 on a strip still renders, and -rayrate 4 through the host layer refuses a strip
    a = G.app(320, 180)
    try:
        a.context.set_strip(0, 90)
        a.OnUpdate(); a.OnRender(); a.context.sync()
        assert a.context.ray_count() > 0
    finally:
        a.OnDestroy()
    a = G.app(320, 180, ["-rayrate", 4])
    try:
        with pytest.raises(capi.RtggxError, match="rtggx_set_strip"):
            a.context.set_strip(0, 90)
        a.OnUpdate(); a.OnRender(); a.context.sync()
        assert a.context.ray_count() > 0
    finally:
        a.OnDestroy()
