"""The lifetime of a context and of what it owns (csrc/rt_owned_hip.h; DESIGN.md "Ownership"): contexts created and destroyed one after
another and side by side with every lazily allocated feature in use, and buffers replaced on a live context -- a mesh by another one,
before and after it has begun to deform; the environment; the ray bins.  Nothing here has a tolerance: whole images are compared word for
word (gpu_support.assert_same) against the same frames of another context.  96x64 frames of the two smallest meshes.

Which images: contexts that went through the same calls agree in everything (ALL).  A context whose mesh or material was replaced is
compared with a fresh one in what a frame writes from its own constants and scene alone (OWN): RayTracingOut1, RoughMetal where nothing
is hit and everything behind the denoiser carry earlier frames' values by design (frame.hip rtggx_ray_trace, rtggx_context.h RT_SKY_PREV_RUN).

rtggx_last_error is per thread and is never cleared, so "no call left an error text" is asserted as "the text is what it was when the
test began" -- empty in a process in which nothing has failed before."""
import numpy as np
import pytest

import assets
import gpu_support as G

pytestmark = pytest.mark.gpu

W, H = 96, 64
SMALL, OTHER = "TuringBowl.obj", "bunny.obj"
ALL = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
OWN = ("vis", "depth", "normal", "velocity", "refl") + G.RAYS
DT = ["-dt", 0.05]


def _error_text(a):
    return a.context.L.rtggx_last_error()


def _mesh(name):
    from raytracedggx_amd import app
    v, i, _ = app.obj_import(assets.path(name))
    return v, i


def _frames(a, n):
    for _ in range(n):
        G.frame(a)


def _round(torch, verts):
    """One context's life with every lazily allocated feature turned on once: (back buffer and all other images, the score records)."""
    a = G.app(W, H, DT, mesh=SMALL)
    quiet = _error_text(a)
    try:
        c = a.context
        steps = []

        def ok(what):
            steps.append(what)
            assert _error_text(a) == quiet, "%s left the error text %r" % (what, _error_text(a))

        c.set_samples_per_pixel(2); ok("samples per pixel")
        c.set_sample_set(512); ok("sample set")
        c.set_accumulation(True); ok("accumulation")
        c.enable_timing(2); ok("timing mode 2")
        G.frame(a); ok("frame 1")
        c.present_accumulation(); ok("present")
        c.reference_from_accumulation(); ok("reference from accumulation")
        c.set_scoring(True); ok("scoring")
        c.refit_as(1, verts); ok("refit_as")
        G.frame(a); ok("frame 2")
        dev = torch.from_numpy(verts).cuda()
        torch.cuda.synchronize()
        c.refit_as_device(1, dev.data_ptr(), verts.shape[0], 0); ok("refit_as_device")
        G.frame(a); ok("frame 3")
        got = G.images(a, ALL); ok("readback")
        scores = c.read_scores(); ok("read scores")
        assert len(c.kernel_times()) > 0; ok("kernel times")
        assert c.refit_stats(1)["refits"] == 2 and c.accumulated_frames() == 3 and len(scores) == 2
        del dev
        return got, scores
    finally:
        a.OnDestroy()
        assert _error_text(a) == quiet


def test_create_render_destroy_three_times_over_with_every_lazy_feature(built):
    import torch
    verts, _ = _mesh(SMALL)
    rounds = [_round(torch, verts) for _ in range(3)]
    assert rounds[0][0]["back"].any() and rounds[0][0]["rays"][0] > 0
    for k in (1, 2):
        G.assert_same(rounds[k][0], rounds[0][0], "round %d against round 0" % k)
        assert repr(rounds[k][1]) == repr(rounds[0][1]), "round %d: score records" % k      # (repr: a NaN equals itself)


def _fresh(mesh, frames, extra=(), before=None):
    """`frames` frames of a context created directly in a state; `before(app)` runs in front of the first one."""
    b = G.app(W, H, DT + list(extra), mesh=mesh)
    try:
        if before:
            before(b)
        _frames(b, frames)
        return {names: G.images(b, names) for names in (ALL, OWN)}
    finally:
        b.OnDestroy()


def test_a_mesh_replaced_on_a_live_context_before_and_after_it_deforms(built):
    """set_mesh + build_as with another mesh on a context that has rendered; the new mesh begins to deform (its own vertices: the shape
    stays), which gives it vertex and tree buffers per input set; then the first mesh again: back to one allocation for all sets."""
    small, other = _mesh(SMALL), _mesh(OTHER)
    a = G.app(W, H, DT, mesh=SMALL)
    quiet = _error_text(a)
    try:
        c = a.context
        _frames(a, 2)
        c.set_mesh(1, *other); c.build_as()
        G.frame(a)
        G.assert_same(G.images(a, OWN), _fresh(OTHER, 3)[OWN], "frame 3, the other mesh")
        c.refit_as(1, other[0])
        G.frame(a)
        assert c.refit_stats(1)["refits"] == 1
        G.assert_same(G.images(a, OWN), _fresh(OTHER, 4)[OWN], "frame 4, the other mesh refitted to its own shape")
        c.set_mesh(1, *small); c.build_as()
        G.frame(a)
        G.assert_same(G.images(a, OWN), _fresh(SMALL, 5)[OWN], "frame 5, the first mesh again")
        c.refit_as(1, small[0])      # and it can begin to deform once more
        G.frame(a)
        G.assert_same(G.images(a, OWN), _fresh(SMALL, 6)[OWN], "frame 6, refitted to its own shape")
        assert _error_text(a) == quiet
    finally:
        a.OnDestroy()


def test_the_environment_loaded_twice_and_the_bins_grown(built):
    """The same environment a second time, through both loaders, replaces the cube on a context in use: every image of the next frame is
    that of a context that loaded it once.  Metallic below 1 after all-metal frames grows the ray bins (frame.hip growBins)."""
    from raytracedggx_amd import capi
    const = assets.constant_env_rgba16f(0.75)
    rng = np.random.default_rng(7)
    pano = rng.uniform(0.0, 2.0, (8, 16, 3)).astype(np.float32)

    def load_const(x):
        x.context.set_env(capi.FORMAT_RGBA16F, 1, 1, const)

    def load_pano(x):
        x.context.set_env_image(capi.ENV_EQUIRECT, capi.PIXELS_RGB32F, 16, 8, pano)

    for load, label in ((load_const, "rtggx_set_env"), (load_pano, "rtggx_set_env_image")):
        a = G.app(W, H, DT, mesh=SMALL)
        quiet = _error_text(a)
        try:
            load(a)
            _frames(a, 2)
            load(a)
            G.frame(a)
            G.assert_same(G.images(a, ALL), _fresh(SMALL, 3, before=load)[ALL], "%s twice" % label)
            assert _error_text(a) == quiet
        finally:
            a.OnDestroy()
    a = G.app(W, H, DT, mesh=SMALL)
    try:
        _frames(a, 2)
        metal = G.images(a, G.RAYS)["rays"][0]
        a.context.set_metallic(1, 0.5)
        G.frame(a)
        want = _fresh(SMALL, 3, before=lambda x: x.context.set_metallic(1, 0.5))[OWN]
        G.assert_same(G.images(a, OWN), want, "diffuse rays after all-metal frames")
        assert want["rays"][0] > metal > 0      # (a second ray per pixel of the mesh: the bins did have to grow)
    finally:
        a.OnDestroy()


_ALONE = {}


def _alone():
    """Four frames of a lone context, once per module."""
    if "images" not in _ALONE:
        got = _fresh(SMALL, 4)[ALL]
        for v in got.values():
            v.setflags(write=False)
        _ALONE["images"] = got
    return _ALONE["images"]


def test_a_context_after_another_one_and_two_side_by_side(built):
    want = _alone()
    G.assert_same(_fresh(SMALL, 4)[ALL], want, "a context after an earlier one has been destroyed")
    a, b = G.app(W, H, DT, mesh=SMALL), G.app(W, H, DT, mesh=SMALL)
    try:
        for _ in range(4):
            G.frame(a); G.frame(b)
        G.assert_same(G.images(a, ALL), want, "first of two contexts alive side by side")
        G.assert_same(G.images(b, ALL), want, "second of two contexts alive side by side")
        a.OnDestroy()      # one goes, the other renders on
        G.frame(b)
        G.assert_same(G.images(b, ALL), _fresh(SMALL, 5)[ALL], "a context whose neighbour has been destroyed")
    finally:
        a.OnDestroy(); b.OnDestroy()
