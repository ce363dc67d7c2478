"""Adaptive sampling on the GPU (rtggx_set_sample_map, rtggx_read_sample_map; include/rtggx.h, DESIGN.md "Adaptive sampling").  Its parity status: no counterpart in the reference.  The mapped frames are pinned bit for bit -- raw images,
G-buffer, ray count, the map read back -- to tests/adaptive_ref.py, which composes them block by block from the CPU restatement's uniform
frames (pinned to the oracle at one sample by the rest of the suite).
The small frame is 100x54: its width is no multiple of 8 or 16, so the last block column and the last bin column are ragged."""
import numpy as np
import pytest

import accum_ref as AR
import adaptive_ref as A
import assets
import gpu_support as G
import score_ref as SR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FRAME_WORDS = G.GBUFFER + G.RAW
IMAGES = FRAME_WORDS + G.DENOISED
SIZES = [(100, 54), (320, 180)]


def maps_for(W, H, N):
    """The maps every configuration is rendered under, in this order on one context: the 1-next-to-8 ones catch a bin that kept its count."""
    by, bx = A.blocks_of(W, H)
    return [("all N", np.full((by, bx), N, np.uint8)), ("all 1", np.ones((by, bx), np.uint8)), ("checkerboard 1 / 8", A.checkerboard(W, H)),
            ("8 in a sea of 1", A.one_in_a_sea(W, H, 1, 8)), ("1 in a sea of 8", A.one_in_a_sea(W, H, 8, 1)),
            ("random", A.random_map(W, H, 7 * W + N))]      # (counts above N included at N = 4: clamped)


def mapped_frame(p, blocks):
    """One frame of a restated Pair under the map in force: the product's frame, then the composition in the pair's oracle."""
    p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
    p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
    p.o.update_as(); p.o.render_visibility()
    p.rays = A.mapped_frame(p.o, blocks)


def run_maps(p, W, H, N, label):
    for name, blocks in maps_for(W, H, N):
        p.ctx.set_sample_map(blocks)
        np.testing.assert_array_equal(p.ctx.read_sample_map(), blocks, err_msg="%s: the map read back" % name)
        mapped_frame(p, blocks)
        G.check_raw(p, "%s, map %s" % (label, name), require_rays=True)


CONFIGS = [
    # W, H, N, mesh, metallic, vndf, depth, sample set
    (100, 54, 8, "bunny.obj", (1.0, 1.0), False, 1, 256),
    (100, 54, 4, "bunny.obj", (0.25, 0.5), True, 1, 256),
    (100, 54, 8, "bunny.obj", (0.25, 0.5), False, 2, 256),
    (100, 54, 4, "bunny.obj", (1.0, 0.75), False, 1, 4096),
    (320, 180, 8, "bunny.obj", (0.25, 0.5), False, 1, 256),
    (320, 180, 4, "bunny.obj", (1.0, 0.75), True, 1, 256),
    (320, 180, 4, "dragon.obj", (0.25, 0.5), False, 1, 256),
]


@pytest.mark.parametrize("W,H,N,mesh,metallic,vndf,depth,sample_set", CONFIGS,
                         ids=["100x54-8-metal", "100x54-4-diffuse-vndf", "100x54-8-diffuse-depth2", "100x54-4-metal-ground-set4096",
                              "320x180-8-diffuse", "320x180-4-metal-ground-vndf", "320x180-4-dragon"])
def test_mapped_frames_equal_the_composition(built, W, H, N, mesh, metallic, vndf, depth, sample_set):
    p = G.restated_pair(W, H, samples=N, depth=depth, sample_set=sample_set, entry="sampleset", mesh=mesh, metallic=metallic, vndf=vndf)
    try:
        run_maps(p, W, H, N, "%s %dx%d N = %d" % (mesh, W, H, N))
    finally:
        p.close()


def test_a_refitted_mesh_under_a_checkerboard(built):
    p = G.restated_pair(100, 54, samples=8, entry="spp", metallic=(1.0, 0.5))
    try:
        blocks = A.checkerboard(100, 54)
        p.ctx.set_sample_map(blocks)
        mapped_frame(p, blocks); G.check_raw(p, "before the deformation")
        v0, idx, _ = O.obj_import(assets.path("bunny.obj"))
        v = G.wave(v0, 1)
        p.ctx.refit_as(1, v)
        p.app.OnUpdate(); p.app.OnRender(); p.ctx.sync()
        p.o.set_mesh(1, v, idx)
        p.give_oracle_the_device_trees(refitted=True)
        p.o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + p.o.get_frame_constants().tobytes()[704:])
        p.o.update_as(); p.o.render_visibility(); p.rays = A.mapped_frame(p.o, blocks)
        G.check_raw(p, "deformed", require_rays=True)
    finally:
        p.close()


@pytest.mark.parametrize("W,H", SIZES, ids=["100x54", "320x180"])
@pytest.mark.parametrize("N", [8, 4])
def test_a_map_of_all_n_is_the_context_that_never_set_one(built, W, H, N):
    """Every buffer through the back buffer, and the ray count, over 4 frames; then the map cleared, and N = 1 with a map set."""
    extra = ["-spp", N, "-metallic", 0.25, 0.5]
    a, b = G.app(W, H, extra), G.app(W, H, extra)
    try:
        a.context.set_sample_map(np.full(A.blocks_of(W, H), N, np.uint8))
        for f in range(4):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES + G.RAYS), G.images(b, IMAGES + G.RAYS), "all %d, frame %d" % (N, f))
        a.context.set_sample_map(A.checkerboard(W, H))
        G.frame(a); G.frame(b)
        assert a.context.ray_count() < b.context.ray_count()
        a.context.set_sample_map(None)
        assert a.context.read_sample_map() is None
        G.frame(a); G.frame(b)
        G.assert_same(G.images(a, FRAME_WORDS + G.RAYS), G.images(b, FRAME_WORDS + G.RAYS), "the map cleared")
        a.context.set_sample_map(A.checkerboard(W, H))
        a.context.set_samples_per_pixel(1); b.context.set_samples_per_pixel(1)
        for f in range(2):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, FRAME_WORDS + G.RAYS), G.images(b, FRAME_WORDS + G.RAYS), "N = 1 ignores the map, frame %d" % f)
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_ray_counts_follow_the_map(built):
    """All 1 < one block raised step by step < ... < all N, each equal to its frame's count; the same frame index every time (a still
    camera, the constants set once)."""
    from raytracedggx_amd import capi
    W, H, N = 100, 54, 8
    a = G.app(W, H, ["-spp", N, "-metallic", 0.25, 0.5])
    try:
        c = a.context
        G.frame(a); c.sync()
        vis = c.readback(capi.BUF_VISIBILITY)
        cov = A.block_lanes(vis != 0, False).sum(axis=-1)
        at = np.unravel_index(np.argmax(cov), cov.shape)
        assert cov[at] > 0

        def rays(blocks):      # the same frame again, from the constants of the frame before
            c.set_sample_map(blocks)
            c.render_visibility(); c.ray_trace(); c.denoise(); c.tone_map(); c.sync()
            return c.ray_count()
        ones, full = np.ones(A.blocks_of(W, H), np.uint8), np.full(A.blocks_of(W, H), N, np.uint8)
        r1, rN = rays(ones), rays(full)
        assert 0 < r1 < rN
        seq = [r1]
        for n in (2, 4, 8):
            m = ones.copy(); m[at] = n
            seq.append(rays(m))
        assert all(x < y for x, y in zip(seq, seq[1:])), seq
        assert seq[-1] < rays(A.checkerboard(W, H)) < rN
        assert rays(None) == rN
    finally:
        a.OnDestroy()


# ---- ordering ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,force_small,own_stream", [(100, 54, 1, False), (320, 180, 0, False), (320, 180, 1, True)],
                         ids=["100x54-small-placement", "320x180-full-size-placement", "320x180-caller-stream"])
def test_free_running_frames_equal_synchronised_ones(built, W, H, force_small, own_stream):
    import torch
    extra = ["-spp", 8, "-metallic", 1.0, 0.5]
    a, b = G.app(W, H, extra), G.app(W, H, extra)
    stream = torch.cuda.Stream() if own_stream else None
    try:
        for x in (a, b):
            x.context.placement(force_small)
        if own_stream:
            b.context.set_stream(stream.cuda_stream)
        changes = {0: A.checkerboard(W, H), 5: A.one_in_a_sea(W, H, 1, 8), 11: A.checkerboard(W, H, 8, 1)}
        for f in range(16):
            if f in changes:
                a.context.set_sample_map(changes[f]); b.context.set_sample_map(changes[f])
            a.OnUpdate(); a.OnRender(); a.context.sync()
            b.OnUpdate(); b.OnRender()
        torch.cuda.synchronize()
        G.assert_same(G.images(a, IMAGES + G.RAYS), G.images(b, IMAGES + G.RAYS), "%dx%d placement %d after 16 frames" % (W, H, force_small))
    finally:
        a.OnDestroy(); b.OnDestroy()


# ---- what reads the mapped words ----------------------------------------------------------------------------------------------------
def test_accumulation_and_scoring_take_the_mapped_words(built):
    from raytracedggx_amd import capi
    W, H, N, metallic = 100, 54, 8, (0.25, 0.5)
    a = G.app(W, H, ["-spp", N, "-metallic", metallic[0], metallic[1]])
    try:
        c = a.context
        ref = np.broadcast_to(np.array([0.5, 0.25, 2.0, 1.0], np.float16).view(np.uint64), (H, W)).copy()
        c.set_reference(ref); c.set_scoring(True); c.set_accumulation(True)
        c.set_sample_map(A.random_map(W, H, 3))
        acc = AR.Accumulator(H, W)
        for f in range(4):
            G.frame(a); c.sync()
            refl, diff, vis = c.readback(capi.BUF_RT_REFL), c.readback(capi.BUF_RT_DIFF), c.readback(capi.BUF_VISIBILITY)
            acc.add(refl, diff, vis, metallic)
            recs = c.read_scores()
            assert len(recs) == 1
            want = SR.score(c.readback(capi.BUF_TSS0 + c.frame_parity()), refl, diff, vis, metallic, ref)
            assert not SR.same_record(recs[0], want), "frame %d: %s" % (f, SR.same_record(recs[0], want))
        assert AR.same_bits(c.readback(capi.BUF_ACC_REFL), acc.refl).all() and AR.same_bits(c.readback(capi.BUF_ACC_DIFF), acc.diff).all()
    finally:
        a.OnDestroy()


def test_tile_words_off_and_still_sky_off_change_nothing(built):
    W, H = 320, 180
    extra = ["-spp", 4, "-metallic", 1.0, 0.5]
    a, b, c = G.app(W, H, extra), G.app(W, H, extra), G.app(W, H, extra)
    try:
        b.context.tile_words(False)
        c.context.static_sky(False)
        for x in (a, b, c):
            x.context.set_sample_map(A.checkerboard(W, H))
        for f in range(12):      # (beyond the still-sky threshold: a's sky tiles are being left alone)
            for x in (a, b, c):
                x.OnUpdate(); x.OnRender()
        ia = G.images(a, IMAGES + G.RAYS)
        G.assert_same(ia, G.images(b, IMAGES + G.RAYS), "tile words off")
        G.assert_same(ia, G.images(c, IMAGES + G.RAYS), "still sky off")
    finally:
        a.OnDestroy(); b.OnDestroy(); c.OnDestroy()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_frame_unchanged(built):
    from raytracedggx_amd import capi
    W, H, N = 100, 54, 4
    extra = ["-spp", N, "-metallic", 0.25, 0.5]
    a, b = G.app(W, H, extra), G.app(W, H, extra)
    by, bx = A.blocks_of(W, H)
    good = A.checkerboard(W, H)
    try:
        for x in (a, b):
            x.context.set_sample_map(good)
        c = a.context

        def refused(call, word):
            with pytest.raises(capi.RtggxError, match=word):
                call()
        for f in range(3):
            refused(lambda: c.set_sample_map(np.ones((by, bx + 1), np.uint8)), "rtggx_set_sample_map")
            refused(lambda: c.set_sample_map(np.ones((by - 1, bx), np.uint8)), "rtggx_set_sample_map")
            refused(lambda: c.set_sample_map(np.ones((bx, by), np.uint8)), "rtggx_set_sample_map")
            for bad in (0, 3, 5, 16, 255):
                m = np.ones((by, bx), np.uint8); m[-1, -1] = bad
                refused(lambda: c.set_sample_map(m), "rtggx_set_sample_map")
            refused(lambda: c.set_strip(8, 40), "rtggx_set_strip")
            np.testing.assert_array_equal(c.read_sample_map(), good)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES + G.RAYS), G.images(b, IMAGES + G.RAYS), "frame %d" % f)
    finally:
        a.OnDestroy(); b.OnDestroy()
    # a strip refuses a map
    x = capi.Context(W, H)
    try:
        x.set_strip(8, 40)
        with pytest.raises(capi.RtggxError, match="rtggx_set_sample_map"):
            x.set_sample_map(good)
        assert x.read_sample_map() is None
        x.set_strip(0, H)
        x.set_sample_map(good)
        x.set_strip(0, H)      # the whole frame is no strip
        x.set_sample_map(None)
        x.set_strip(8, 40)
    finally:
        x.close()
