"""What the GPU tests share: the product's application object beside an oracle (Pair) and its frame check, the application-level helpers
of the tests that compare two contexts (app, frame, images, assert_same), the raw check against a restatement (restated_pair, check_raw),
a rate-4 frame against the full-rate one (quad_frame, check_quad_frame), the strips exchanging through RCCL, and the bare context beside
an oracle that the BVH tests trace rays through (Scene, model_box, interval_edges).  raytracedggx_amd is imported inside the functions:
importing this module needs no GPU and no built library."""
import numpy as np

import assets
import bvh_cases
import bvh_checks
import env_cases
import ray_rate_ref as R
from oracle import oracle as O

FRAME_INDEX_OFFSET = 444      # RtggxCBGlobal::FrameIndex in the 768 bytes of RtggxFrameConstants (include/rtggx.h): the last word of `global`, word 111

HDR_TOL = 1e-3   # relative L2, from north_star
# ... against the oracle's EXACT evaluation of the filters' normal weight pow(dot(N, Nc), 512).  Against its plain-fp32 reading of the HLSL
# ("libm": fp32 dot product, std::pow in fp32) the bar is wider, and stated here rather than met by sharing a rounding: ONE fp32 rounding of
# a dot product next to 1 is 6e-8, times 512 in the weight = 3e-5 -- what any two faithful fp32 implementations of the shader differ by
# (HLSL fixes neither the order of a dp3 nor the last bits of pow) --, and the temporal pass turns a 1e-5 difference of the filtered image into
# 1e-3 of its result (measured: 1.03e-3 on the 1080p bunny, frame 1).  The product evaluates the exact value to a few ulps.
HDR_TOL_FP32_ORACLE = 2e-3


class _DeviceView:
    """A raw device pointer through __cuda_array_interface__ (torch wraps it without a copy)."""
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 3}


def rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


# what a frame's check compares bit for bit, product against oracle: (name, the buffer id's name in capi and in oracle.py)
GBUFFER_WORDS = (("visibility", "BUF_VISIBILITY"), ("depth", "BUF_DEPTH"), ("normal", "BUF_NORMAL"), ("roughMetal", "BUF_ROUGH_METAL"), ("velocity", "BUF_VELOCITY"))
# the raw traced images: bit for bit since round 3 (the shading path's exp2 / log2 are the numeric contract's on both sides,
# rtggx_device.h exp2Contract / log2Contract; until then a word could differ by one code)
RAW_WORDS = (("rt_refl", "BUF_RT_REFL"), ("rt_diff", "BUF_RT_DIFF"))


def _assert_words(p, label, table):
    for name, bid in table:
        np.testing.assert_array_equal(p.ctx.readback(getattr(p.capi, bid)), p.o.buffer(getattr(O, bid)), err_msg="%s: %s not bit-exact" % (label, name))


class Pair:
    """The product's RayTracedGGX application object and an oracle on the same scene."""

    def __init__(self, W, H, mesh="bunny.obj", metallic=None, pos_scale=None, env_const=None, shared_mem=False, normal_weight="exact", env=None, oracle=None):
        """oracle: a callable (W, H) -> Oracle in place of O.Oracle (restated_pair)."""
        from raytracedggx_amd import app, capi
        self.capi = capi
        args = ["-mesh", assets.path(mesh)] + ([str(x) for x in pos_scale] if pos_scale else []) + \
               ["-env", assets.path("rnl_cross.dds"), "-width", W, "-height", H]
        if metallic is not None:
            args += ["-metallic", metallic[0], metallic[1]]
        if shared_mem:
            args += ["-sharedmem"]          # the [V] toggle of the sample: LDS-staged spatial filters
        self.app = app.RayTracedGGX(args)
        self.ctx = self.app.context
        self.o = (oracle or O.Oracle)(W, H)
        # how the oracle evaluates the filters' pow(dot(N, Nc), 512): "exact" (double, rounded once) or "libm" (a plain fp32 reading of the
        # HLSL) -- neither shares a rounding with the product's v_exp_f32(512 v_log_f32 x) (oracle/orc_denoise.h normal_weight; process-wide)
        self.o.set_normal_weight(normal_weight)
        v, i, _ = O.obj_import(assets.path(mesh))
        self.o.set_mesh(1, v, i)
        if pos_scale:
            self.o.set_pos_scale(pos_scale)
        if env_const is not None:
            env = assets.constant_env_rgba16f(env_const)
            self.ctx.set_env(capi.FORMAT_RGBA16F, 1, 1, env)
            self.o.set_env_rgba16f(1, 1, env)
        elif env is not None:      # (size, mips, per level the RGBA16F codes [6, s, s, 4]): tests/env_cases.py
            cube = env_cases.Cube(env[0], env[1], env[2], "env")
            self.ctx.set_env(capi.FORMAT_RGBA16F, cube.size, cube.mips, cube.dds_order())
            self.o.set_env_rgba16f(cube.size, cube.mips, cube.mip_major())
        else:
            self.o.set_env_dds(assets.path("rnl_cross.dds"))
        if metallic is not None:
            self.o.set_metallic(0, metallic[0]); self.o.set_metallic(1, metallic[1])
        self.hdr_tol = HDR_TOL if normal_weight == "exact" else HDR_TOL_FP32_ORACLE
        self.num_tris = [12, i.size // 3]
        self.give_oracle_the_device_trees()
        self.o.transform_sh()
        self.rays = None

    def give_oracle_the_device_trees(self, refitted=False):
        """The CPU re-traces the same BVH arrays the HIP kernels use -- after checking them: every primitive in exactly one
        leaf with its own vertices (the oracle's copy of the mesh), every box tight around what is below it, the 4-wide collapse equal to the binary tree and chosen by the surface-area
        rule (tests/bvh_checks.py; refitted: the model's tree keeps the choice its build made for another shape)."""
        capi = self.capi
        for slot, (bn, bt, b4, btop, cap) in enumerate(((capi.BUF_BVH_NODES0, capi.BUF_BVH_TRIS0, capi.BUF_BVH4_NODES0, capi.BUF_BVH4_TOP0, 16),
                                                        (capi.BUF_BVH_NODES1, capi.BUF_BVH_TRIS1, capi.BUF_BVH4_NODES1, capi.BUF_BVH4_TOP1, 96))):
            nodes, tris, root = self.ctx.readback(bn), self.ctx.readback(bt), self.ctx.bvh_root(slot)
            bvh_checks.bvh_check(nodes, tris, root, self.num_tris[slot], *self.o.mesh(slot))
            nodes4 = self.ctx.readback(b4)
            bvh_checks.bvh4_check(nodes, nodes4, root, built_shape=not (refitted and slot == 1), weights=self.ctx.collapse_weights())
            bvh_checks.bvh4_top_check(nodes4, self.ctx.readback(btop), root, cap)
            self.o.set_bvh(slot, nodes, tris, root)

    def frame(self):
        self.app.OnUpdate(); self.app.OnRender(); self.ctx.sync()
        # the oracle consumes the constants the product's host layer produced (its own are checked in test_host_and_abi)
        self.o.set_frame_constants(self.app.frame_constants().tobytes()[:704] + self.o.get_frame_constants().tobytes()[704:])
        self.o.update_as(); self.o.render_visibility(); self.rays = self.o.ray_trace(); self.o.denoise(); self.o.tone_map()

    def close(self):
        self.app.OnDestroy(); self.o.close()

    def check_frame(self, label):
        capi, ctx, o = self.capi, self.ctx, self.o
        _assert_words(self, label, GBUFFER_WORDS)
        np.testing.assert_array_equal(ctx.readback(capi.BUF_TLAS), o.inv_worlds())
        assert ctx.ray_count() == self.rays, "%s: ray count" % label
        _assert_words(self, label, RAW_WORDS)
        p = ctx.frame_parity()
        assert p == o.parity()
        for name, gid, oid in (("FilteredOut", capi.BUF_FLT_RFL, O.BUF_FLT_RFL), ("FilteredOut1", capi.BUF_FLT_DFF, O.BUF_FLT_DFF),
                               ("TemporalSSOut", capi.BUF_TSS0 + p, O.BUF_TSS0 + p)):
            g, r = O.unpack_rgba16f(ctx.readback(gid)), O.unpack_rgba16f(o.buffer(oid))
            # NaNs are part of the reference's behaviour near the frame border (0 x inf in ReflectionWeight for taps that
            # read outside the image, SpatialFilter.hlsli:60): they must appear in the same pixels, nowhere else
            fin = np.isfinite(r)
            np.testing.assert_array_equal(np.isfinite(g), fin, err_msg="%s: %s non-finite values differ from the oracle's" % (label, name))
            e = rel_l2(np.where(fin, g, 0.0), np.where(fin, r, 0.0))
            assert e < self.hdr_tol, "%s: %s relative L2 %.3e" % (label, name, e)
        g, r = O.unpack_rgba8(ctx.readback(capi.BUF_BACKBUFFER)).astype(int), O.unpack_rgba8(o.buffer(O.BUF_BACKBUFFER)).astype(int)
        # 8-bit codes: a value on a rounding boundary may land on either side (the denoiser uses v_rcp/v_sqrt where the
        # oracle divides); never more than one code, rarely, and far inside the 1e-3 bar as an image
        assert np.abs(g - r).max() <= 1 and (g != r).mean() < 2e-2 and rel_l2(g, r) < HDR_TOL, "%s: back buffer" % label


def check_raw(p, label, require_rays=False):
    """G-buffer words, RayTracingOut0/1 and the ray count of a Pair's frame: bit for bit / equal (require_rays: and not zero)."""
    _assert_words(p, label, GBUFFER_WORDS + RAW_WORDS)
    assert p.ctx.ray_count() == p.rays, "%s: ray count %d, restatement %d" % (label, p.ctx.ray_count(), p.rays)
    assert p.rays > 0 or not require_rays, "%s: no ray traced" % label


def restated_pair(W, H, *, depth=1, samples=1, sample_set=256, entry="sampleset", mesh="bunny.obj", metallic=None, vndf=False, shared_mem=False):
    """A Pair with a restatement (tests/restatement.py, its C function `entry`) as its oracle, both at `depth`, `samples` and `sample_set`."""
    import restatement as RS
    p = Pair(W, H, mesh=mesh, metallic=metallic, shared_mem=shared_mem,
             oracle=lambda w, h: RS.Oracle(w, h, depth=depth, samples=samples, sample_set=sample_set, entry=entry))
    if entry == "sampleset":
        p.ctx.set_sample_set(sample_set)
    if samples != 1:
        p.ctx.set_samples_per_pixel(samples)
    if depth != 1:
        p.ctx.set_max_recursion_depth(depth)
    if vndf:
        p.ctx.set_sampler(True); p.o.set_sampler(True)
    return p


# ---- two contexts side by side ---------------------------------------------------------------------------------------------------------
def app(W, H, extra=(), mesh="bunny.obj"):
    from raytracedggx_amd import app
    return app.RayTracedGGX(["-mesh", assets.path(mesh), "-env", assets.path("rnl_cross.dds"), "-width", W, "-height", H] + list(extra))


def frame(a):
    a.OnUpdate(); a.OnRender()


def frame_index(a):
    return int(a.frame_constants()[FRAME_INDEX_OFFSET:FRAME_INDEX_OFFSET + 4].view(np.uint32)[0])


# What images() reads back, in groups.  Every module names the selection it has always compared.  Known reasons for a narrow one: a rate-4
# and a rate-1 frame, or a strip and the whole frame, trace different numbers of rays (no "rays"); the rows of a strip and contexts whose
# histories differ agree in the frame's own words only (no DENOISED).  For GBUFFER_MIN (the recursion and samples-per-pixel tests, which
# leave out depth and velocity) no reason is recorded.
_IMAGE_IDS = {"vis": "BUF_VISIBILITY", "depth": "BUF_DEPTH", "normal": "BUF_NORMAL", "rm": "BUF_ROUGH_METAL", "velocity": "BUF_VELOCITY",
              "refl": "BUF_RT_REFL", "diff": "BUF_RT_DIFF", "flt_rfl": "BUF_FLT_RFL", "flt_dff": "BUF_FLT_DFF", "tss0": "BUF_TSS0", "tss1": "BUF_TSS1",
              "back": "BUF_BACKBUFFER"}
GBUFFER_MIN = ("vis", "normal", "rm")
GBUFFER = ("vis", "depth", "normal", "rm", "velocity")
RAW = ("refl", "diff")
DENOISED = ("flt_rfl", "flt_dff", "tss0", "tss1", "back")
RAYS = ("rays",)      # the ray count, as an array of one


def gbuffer(ctx):
    """The G-buffer of a context that has been waited for."""
    from raytracedggx_amd import capi
    return {n: ctx.readback(getattr(capi, _IMAGE_IDS[n])) for n in GBUFFER}


def images(a, names):
    """The buffers `names` of the application's context, by name; synchronises first."""
    from raytracedggx_amd import capi
    c = a.context
    c.sync()
    return {n: np.array([c.ray_count()]) if n == "rays" else c.readback(getattr(capi, _IMAGE_IDS[n])) for n in names}


def assert_same(a, b, label):
    assert a.keys() == b.keys(), "%s: %s against %s" % (label, sorted(a), sorted(b))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s differs" % (label, k))


# ---- a rate-4 frame against the full-rate one (tests/ray_rate_ref.py) -----------------------------------------------------------------
def quad_frame(p, give_oracle_raw=True):
    """One frame of a rate-4 Pair: the product's frame, the oracle's full-rate frame up to its raw images (returned), which are then
    replaced by the product's reconstructed ones before the oracle denoises and tone-maps."""
    capi, ctx, o = p.capi, p.ctx, p.o
    p.app.OnUpdate(); p.app.OnRender(); ctx.sync()
    o.set_frame_constants(p.app.frame_constants().tobytes()[:704] + o.get_frame_constants().tobytes()[704:])
    o.update_as(); o.render_visibility(); p.rays = o.ray_trace()
    full = {"refl": o.buffer(O.BUF_RT_REFL), "diff": o.buffer(O.BUF_RT_DIFF)}
    if give_oracle_raw:
        o.buffer(O.BUF_RT_REFL, copy=False)[...] = ctx.readback(capi.BUF_RT_REFL)
        o.buffer(O.BUF_RT_DIFF, copy=False)[...] = ctx.readback(capi.BUF_RT_DIFF)
    o.denoise(); o.tone_map()
    return full


def check_quad_frame(p, full, label, prev_diff=None):
    """Test 1 and 2 on one rate-4 frame: G-buffer bit-exact everywhere; raw images bit-exact at traced (where a ray of that kind is
    traced) and background pixels; ray count a quarter; the untraced covered pixels equal their restatement to one code on <= 0.1 %;
    carried-over RayTracingOut1 equal to the previous frame's."""
    capi, ctx, o = p.capi, p.ctx, p.o
    g = gbuffer(ctx)
    for name, oid in (("vis", O.BUF_VISIBILITY), ("depth", O.BUF_DEPTH), ("normal", O.BUF_NORMAL), ("rm", O.BUF_ROUGH_METAL), ("velocity", O.BUF_VELOCITY)):
        np.testing.assert_array_equal(g[name], o.buffer(oid), err_msg="%s: %s not bit-exact" % (label, name))
    H, W = g["vis"].shape
    fi = frame_index(p.app)
    traced = R.traced_mask(W, H, fi)
    covered = g["vis"] != 0
    metal = (g["rm"] >> 8) >= 255
    refl, diff = ctx.readback(capi.BUF_RT_REFL), ctx.readback(capi.BUF_RT_DIFF)
    rays = ctx.ray_count()
    assert 0.2 * p.rays <= rays <= 0.3 * p.rays, "%s: %d rays against %d at full rate" % (label, rays, p.rays)
    at = traced | ~covered
    np.testing.assert_array_equal(refl[at], full["refl"][at], err_msg="%s: RayTracingOut0 at traced / background pixels" % label)
    at_d = (traced & covered & ~metal) | ~covered
    np.testing.assert_array_equal(diff[at_d], full["diff"][at_d], err_msg="%s: RayTracingOut1 at traced / background pixels" % label)
    inst = np.where(covered, (g["vis"].astype(np.int64) - 1) >> 24, -1)
    diffuse_instances = sorted(set(inst[covered & ~metal].tolist()))
    er, ed, target, dif = R.reconstruct(g["vis"], g["depth"], g["normal"], g["rm"], refl, diff, fi, diffuse_instances)
    assert target.sum() > 0
    for name, got, want, mask in (("RayTracingOut0", refl, er, target), ("RayTracingOut1", diff, ed, dif)):
        if not mask.any():
            continue
        a, b = got[mask].astype(np.int64), want[mask].astype(np.int64)
        d = np.stack([np.abs((a & 0x7FF) - (b & 0x7FF)), np.abs(((a >> 11) & 0x7FF) - ((b >> 11) & 0x7FF)), np.abs((a >> 22) - (b >> 22))])
        assert d.max() <= 1 and (d.max(axis=0) > 0).mean() <= 1e-3, "%s: reconstructed %s: %d of %d pixels differ, by up to %d codes" % (
            label, name, int((d.max(axis=0) > 0).sum()), a.size, int(d.max()))
    if prev_diff is not None:
        carry = covered & metal
        np.testing.assert_array_equal(diff[carry], prev_diff[carry], err_msg="%s: RayTracingOut1 carried over" % label)
    return diff


# ---- strips ----------------------------------------------------------------------------------------------------------------------------
def strips_through_rccl_equal_the_full_frame(W, H, world, balance, frames, mesh="bunny.obj", extra=(), peers=True, overreach=None):
    """`world` strips of one process, each its own context, exchanging through the direct RCCL path (raytracedggx_amd/rccl.py:
    ncclSend/ncclRecv in one group on the renderer's stream, pointers from StripRenderer.raw_ops) on the one GPU of the box: a
    single-rank communicator whose sends and receives pair up with each other -- against the single-context frame.  (Across
    processes the only difference is the peer number.)  peers: every strip maps every strip's history images (rtggx_set_history_peers,
    round 4), and the exchange carries the ordering tokens.  overreach: a list that receives, per frame, the largest number of rows by
    which a history tap of any strip read beyond the exchanged apron."""
    import torch
    from raytracedggx_amd import capi, rccl
    from raytracedggx_amd.strips import HISTORY_APRON, StripRenderer
    mesh, env = assets.path(mesh), assets.path("rnl_cross.dds")
    strips = []
    comm = rccl.Communicator(None, 0, 1)

    def transport(r, plan):
        ops = []
        for op, name, r0, r1, peer in plan:
            if op == "recv":
                src = strips[peer]
                ops += src.raw_ops([("send", name, r0, r1, 0)], src.context.frame_parity())
                ops += r.raw_ops([("recv", name, r0, r1, 0)], r.context.frame_parity())
        for t in strips:
            r.xstream.wait_stream(t.xstream); r.xstream.wait_stream(t.stream)
        comm.exchange(ops, r.xstream.cuda_stream)

    full = StripRenderer(W, H, mesh, env, extra_args=("-sharedmem",) + tuple(extra))
    strips += [StripRenderer(W, H, mesh, env, rank=r, world=world, transport=transport, torch_buffers=True, extra_args=("-sharedmem",) + tuple(extra), balance=balance, peers=peers) for r in range(world)]
    for t in strips:
        t.connect_peers(strips)
    if balance is True:
        assert all(s.bounds == strips[0].bounds for s in strips) and strips[0].bounds != [(r * H) // world for r in range(world + 1)]
        for _ in range(StripRenderer.PROFILE_FRAMES):          # the strips have rendered these as whole frames: the reference follows
            full.frame()
    try:
        for f in range(frames):
            full.frame()
            for s in strips:
                s.render()
            for s in strips:
                s.exchange()
            for s in strips:
                for t in strips:
                    s.stream.wait_stream(t.stream); s.stream.wait_stream(t.xstream)
            torch.cuda.synchronize(); full.context.sync()
            if overreach is not None:
                overreach.append(max(t.history_overreach(reset=True) for t in strips))
            np.testing.assert_array_equal(strips[0].context.readback(capi.BUF_BACKBUFFER), full.context.readback(capi.BUF_BACKBUFFER), err_msg="frame %d" % f)
            bid = capi.BUF_TSS1 if full.context.frame_parity() else capi.BUF_TSS0
            ref = full.context.readback(bid)
            for k, s in enumerate(strips):          # each strip's history, with the apron rows it received, equals the full frame's
                lo, hi = max(s.b - HISTORY_APRON, 0), min(s.e + HISTORY_APRON, H)
                assert s.context.frame_parity() == full.context.frame_parity()
                np.testing.assert_array_equal(s.context.readback(bid)[lo:hi], ref[lo:hi], err_msg="history of strip %d, frame %d" % (k, f))
        assert sum(s.context.ray_count() for s in strips) == full.context.ray_count(), "rays are counted once, by the strip that owns the pixel"
        return full.context.ray_count()
    finally:
        comm.destroy()
        full.close()
        for s in strips:
            s.close()


def wave(v0, f, amp=0.35):
    v = v0.copy()
    v[:, 0] += amp * np.sin(1.3 * v0[:, 1] + 0.9 * f)
    v[:, 2] += 0.7 * amp * np.cos(0.8 * v0[:, 1] - 0.7 * f)
    return v


# ---- a bare context beside an oracle, for rays through synthetic meshes (tests/bvh_cases.py) -----------------------------------------
BVH_SETS = ((("BUF_BVH_NODES0", "BUF_BVH_TRIS0", "BUF_BVH4_NODES0", "BUF_BVH4_TOP0"), 16), (("BUF_BVH_NODES1", "BUF_BVH_TRIS1", "BUF_BVH4_NODES1", "BUF_BVH4_TOP1"), 96))


class Scene:
    """A capi.Context and an oracle holding the same two meshes and instance transforms.  camera: the frame constants are an ordinary
    camera's (the oracle's default one) with the scene's Worlds, for the tests that run frames (frame): the visibility pass then sees
    ordinary input.  built_shape: see check_trees, for the check of the build.  size: (W, H) of both (default: the BVH tests' 64 x 64);
    oracle: a callable (W, H) -> Oracle in place of O.Oracle."""

    def __init__(self, mesh0, mesh1, world0=None, world1=None, camera=False, built_shape=True, size=None, oracle=None):
        from raytracedggx_amd import capi
        self.capi = capi
        self.meshes = [mesh0, mesh1]
        self.worlds = [bvh_cases.world(4.0, (0.0, -6.0, 0.0)) if world0 is None else world0, bvh_cases.world() if world1 is None else world1]
        self.W, self.H = size or (bvh_cases.W, bvh_cases.H)
        self.ctx = capi.Context(self.W, self.H)
        self.o = (oracle or O.Oracle)(self.W, self.H)
        try:
            for slot, (v, i) in enumerate(self.meshes):
                self.ctx.set_mesh(slot, v, i)
                self.o.set_mesh(slot, v, i)
            self.ctx.build_as()
            base = None
            if camera:
                self.o.update_frame((10, 10, -24), O.camera_view_proj(self.W, self.H), 0.0)
                base = self.o.get_frame_constants()
            self.fc = bvh_cases.frame_constants(*self.worlds, base=base)
            self.ctx.update_frame(self.fc); self.ctx.update_as()
            self.o.set_frame_constants(self.fc); self.o.update_as()
            np.testing.assert_array_equal(self.ctx.readback(capi.BUF_TLAS), self.o.inv_worlds())
            self.depth = self.check_trees(built_shape)
        except Exception:
            self.close()
            raise

    def close(self):
        self.ctx.close(); self.o.close()

    def arrays(self, slot):
        """(nodes, tris, nodes4, top) of the slot's tree in the current input set, and its root."""
        return tuple(self.ctx.readback(getattr(self.capi, b)) for b in BVH_SETS[slot][0]), self.ctx.bvh_root(slot)

    def check_trees(self, built_shape=True):
        """Structure of both trees (leaf vertices, tight boxes, the 4-wide collapse, the LDS tables of 16 and 96 nodes); then the
        oracle gets the device's arrays for the tree-walk comparison.  built_shape: the collapse is the one the surface-area rule gives
        for this shape (a bool, or one per slot: a refitted tree keeps the choice its build made for another shape).  Returns the binary
        depth of each tree (self.tops: the entries of each table)."""
        depth, self.tops = [], []
        built = (built_shape, built_shape) if isinstance(built_shape, bool) else built_shape
        for slot in range(2):
            v, i = self.meshes[slot]
            (nodes, tris, nodes4, top), root = self.arrays(slot)
            depth.append(bvh_checks.bvh_check(nodes, tris, root, i.size // 3, v, i))
            bvh_checks.bvh4_check(nodes, nodes4, root, built_shape=built[slot], weights=self.ctx.collapse_weights())
            self.tops.append(bvh_checks.bvh4_top_check(nodes4, top, root, BVH_SETS[slot][1]))
            self.o.set_bvh(slot, nodes, tris, root)
        return depth

    def frame(self, shapes=None, device=False):
        """One frame as far as a refit needs it: update_frame + update_as + render_visibility + sync (rtggx_render_visibility is where a
        staged shape is uploaded and the tree refitted; a frame without the later passes is supported).  shapes: {slot: verts} handed to
        refit_as first, and to the oracle as the slot's mesh."""
        for slot, v in (shapes or {}).items():
            self.ctx.refit_as(slot, v)
            self.set_shape(slot, v)
        self.ctx.update_frame(self.fc); self.ctx.update_as(); self.ctx.render_visibility(); self.ctx.sync()

    def set_cube(self, cube, vndf=False):
        """The same environment (an env_cases.Cube) and sampler on both sides.  The nine SH coefficients are projected on each side by its own
        code (tests/test_gpu_env.py holds the device's to the float64 projection); the oracle then takes the device's, so that a frame's words
        compare bit for bit whatever the last bit of a coefficient."""
        self.ctx.set_env(self.capi.FORMAT_RGBA16F, cube.size, cube.mips, cube.dds_order())
        self.o.set_env_rgba16f(cube.size, cube.mips, cube.mip_major())
        np.testing.assert_array_equal(self.ctx.readback(self.capi.BUF_ENV), cube.mip_major())
        self.ctx.transform_sh(); self.o.transform_sh()
        dev, own = self.ctx.readback(self.capi.BUF_SH_COEFFS).reshape(9, 3), self.o.buffer(O.BUF_SH_COEFFS)
        np.testing.assert_allclose(dev, own, rtol=1e-5, atol=1e-6)      # (gross errors only, the frames' own tolerance in tests/test_gpu_parity.py; the bound that
        # holds the projection is tests/test_gpu_env.py's: 2^-23 of each coefficient's magnitude against the float64 sum)
        self.o.set_sh(dev)
        self.ctx.set_sampler(bool(vndf)); self.o.set_sampler(bool(vndf))

    def shaded_frame(self, constants, materials, strip=None):
        """One frame up to the traced images on both sides: materials ((colour, roughness, metallic) per instance), the 768 bytes, the
        instance transforms, visibility, ray generation and tracing.  strip: (first row, end row) of the device's frame.
        -> (the device's words by the names of gbuffer() and RAW, its ray count, the oracle's ray count)."""
        for slot, (colour, rough, metal) in enumerate(materials):
            self.ctx.set_material(slot, colour, rough, metal)
        if strip:
            self.ctx.set_strip(*strip)
        self.fc = bytes(constants)
        self.ctx.update_frame(self.fc); self.ctx.update_as(); self.ctx.render_visibility(); self.ctx.ray_trace(); self.ctx.sync()
        self.o.set_frame_constants(self.fc); self.o.update_as(); self.o.render_visibility()
        rays = self.o.ray_trace()
        words = {n: self.ctx.readback(getattr(self.capi, _IMAGE_IDS[n])) for n in GBUFFER + RAW}
        return words, self.ctx.ray_count(), rays

    def set_shape(self, slot, v):
        """The oracle's (and the checks') copy of a slot's vertices."""
        self.meshes[slot] = (np.array(v, np.float32), self.meshes[slot][1])
        self.o.set_mesh(slot, *self.meshes[slot])

    def compare(self, rays, label, min_hits=0):
        """HIP traversal == oracle brute force == oracle walking the device tree, bit for bit."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        g = self.ctx.trace_rays(rays)
        b = self.o.trace_rays(rays, brute=True)
        w = self.o.trace_rays(rays)
        for other, what in ((b, "brute force"), (w, "oracle walking the device tree")):
            bad = np.nonzero(g["valid"] != other["valid"])[0]
            assert bad.size == 0, "%s: %d rays hit on one side only (vs %s), first ray %d: %s, device %s" % (
                label, bad.size, what, bad[0], rays[bad[0]].tolist(), bool(g["valid"][bad[0]]))
            hit = other["valid"]
            for k in ("inst", "prim", "t", "b1", "b2"):
                a, c = g[k][hit].view(np.uint32), other[k][hit].view(np.uint32)
                bad = np.nonzero(a != c)[0]
                assert bad.size == 0, "%s: %s differs (vs %s) on %d rays, first ray %d: device %s, oracle %s" % (
                    label, k, what, bad.size, np.nonzero(hit)[0][bad[0]], g[k][hit][bad[0]], other[k][hit][bad[0]])
        assert b["valid"].sum() >= min_hits, "%s: only %d of %d rays hit" % (label, b["valid"].sum(), len(rays))
        return b


def model_box(scene, slot=1):
    """World-space box of a mesh (the instance transforms here are scale, quarter turn and translation: corners suffice)."""
    return bvh_cases.world_box(scene.meshes[slot][0], scene.worlds[slot])


def interval_edges(scene, rays, label):
    """Rays that hit again, with tmax, then tmin, set to the exact t of their closest hit (both bounds are exclusive: the hit at
    that t must go, on both sides alike), and with empty intervals (tmin == tmax, tmin > tmax: nothing hits)."""
    b = scene.o.trace_rays(rays, brute=True)
    hit = rays[b["valid"]].copy()
    t = b["t"][b["valid"]]
    if hit.shape[0]:
        at_tmax = hit.copy(); at_tmax[:, 7] = t
        scene.compare(at_tmax, label + ", tmax = t of the closest hit")
        at_tmin = hit.copy(); at_tmin[:, 6] = t
        scene.compare(at_tmin, label + ", tmin = t of the closest hit")
        empty = hit.copy(); empty[:, 6] = t; empty[:, 7] = t
        g = scene.ctx.trace_rays(empty)
        assert not g["valid"].any(), label + ": an empty interval hit"
        rev = hit.copy(); rev[:, 6] = t; rev[:, 7] = t * np.float32(0.5)
        assert not scene.ctx.trace_rays(rev)["valid"].any(), label + ": tmin > tmax hit"
