"""The deforming-mesh path on small synthetic meshes: rtggx_refit_as / rtggx_refit_as_device, the per-set vertex and tree buffers, the
refit kernels (csrc/lbvh.hip refitTris, refitTreelets, emitNodes, emitNodes4, emitTop, treeCostKernel) and the cost-driven rebuild beside
the frames (startRebuild, continueRebuild, abandonRebuild, the topology swap).

A refit has no rounding, so what it must leave is known exactly: tests/refit_ref.py computes it from the arrays before the refit and
the new vertices, and every frame here is checked three ways (check_after_refit): (i) the device's four arrays against that model --
references, ids and leaf vertices bit for bit, boxes as values; (ii) the structure checks of tests/bvh_checks.py; (iii) the HIP
traversal against the oracle's BRUTE FORCE over the moved triangles and against the oracle walking the device's arrays, bit for bit
(a box that loses a triangle shows against the first).  tests/test_refit_ref_host.py checks the model itself, and that the ray sets
used here reach the deformed meshes, on the host.

A frame is update_frame + update_as + render_visibility + sync (gpu_support.Scene.frame): rtggx_render_visibility is where a staged
shape is uploaded and the tree refitted; after the sync, readback and trace_rays see the current input set's tree (rtggx_context.h
selectSet sets MeshDev::nodes / nodes4 / tris / top, which debug.hip bufferInfo and trace.hip launchTrace read)."""
import numpy as np
import pytest

import bvh_cases as BC
import bvh_checks
import refit_ref
from gpu_support import Scene

pytestmark = pytest.mark.gpu

NO_REBUILD = 1e30        # a cost ratio no shape reaches (1e30 x the build's cost overflows to +inf): the topology under test stays
# Launches of one rebuild beside the frames of a mesh of 2 .. 2048 triangles (lbvh.hip planBuildSteps): the snapshot copy, buildBegin,
# boundsKernel, mortonKernel, 4 x 4 of the radix sort, plocInit, no multi-workgroup round (plocRoundsFor: none up to RT_PLOC_STOP = 2048
# triangles), plocFinal, leafRank, leafPermute, 2 copies, 2 x 3 for the treelets, the memset of topRank, 3 x collapseCostTreelets,
# entries4, roots4, planTop, depth, treeCost, the copy of the result: 42.
REBUILD_STEPS = 42


def same_bits(got, want, label):
    for name, g, w in zip(("binary nodes", "leaf triangles", "4-wide nodes", "top table"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differ from the build's, bit for bit" % (label, name)


def structure_and_hits(scene, slots, label, min_hits=1, refitted=(0, 1)):
    """(ii) and (iii) for the scene as it stands; the rays go through the box of each slot in `slots` and at its vertices."""
    scene.check_trees(built_shape=tuple(k not in refitted for k in (0, 1)))
    hits = {}
    for slot in slots:
        v, idx = scene.meshes[slot]
        b = scene.compare(BC.refit_rays(v, scene.worlds[slot], seed=idx.size // 3), label)
        own = b["valid"] & (b["inst"] == slot)
        assert own.sum() >= min_hits, "%s: %d rays hit the mesh in slot %d" % (label, own.sum(), slot)
        hits[slot] = b
    return hits


def check_after_refit(scene, before, verts, label, min_hits=1):
    """before: {slot: ((nodes, tris, nodes4, top), root)} read from any input set that holds the topology; verts: {slot: the shape the
    current set must now show}.  (i), (ii), (iii) of the module's text."""
    for slot, v in verts.items():
        arrays, root = before[slot]
        got, got_root = scene.arrays(slot)
        assert got_root == root
        refit_ref.same_arrays(got, refit_ref.refit_expect(*arrays, root, v, scene.meshes[slot][1]), "%s, slot %d" % (label, slot))
    return structure_and_hits(scene, tuple(verts), label, min_hits, refitted=tuple(verts))


# ---- a. sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot,n", [(1, n) for n in BC.SLOT1_SIZES] + [(0, n) for n in BC.SLOT0_SIZES])
def test_refit_across_sizes(built, slot, n):
    """1 triangle: no node at all; 2: one node, a cost over a single box; slot 0: a table of 16; 1026: 1025 nodes, the first tree whose
    root is a level-1 treelet of one item; 2049 / 3073: the build's multi-workgroup rounds.  Six frames through three shapes, two of
    them without a new shape (the set they use must show the newest one: the other sets' vertex buffers follow), then back to the
    build's shape: the arrays of emit-after-refit equal those of emit-after-build bit for bit, the zeroed unused 4-wide slots included."""
    s = Scene(*BC.refit_scene(slot, n), camera=True)
    try:
        s.ctx.set_refit_policy(NO_REBUILD, 16)
        if slot == 0 and n >= 97:
            assert s.tops[0] == 16
        v0 = s.meshes[slot][0]
        built_ = {slot: s.arrays(slot)}
        a, b, c = BC.size_shapes(v0)
        for f, shape in enumerate((a, b, None, None, c, b)):
            s.frame({slot: shape} if shape is not None else None)
            check_after_refit(s, built_, {slot: s.meshes[slot][0]}, "slot %d, %d triangles, frame %d" % (slot, n, f))
        s.frame({slot: v0})
        same_bits(s.arrays(slot)[0], built_[slot][0], "slot %d, %d triangles, back at the build's shape" % (slot, n))
        st = s.ctx.refit_stats(slot)
        assert st["refits"] == 7 and st["rebuilds"] == 0, st
    finally:
        s.close()


# ---- b. deformations ---------------------------------------------------------------------------------------------------------------
def _deformation_scene(mesh):
    if mesh == "grid":
        return Scene(BC.mesh_from_tris(BC.soup(12, seed=100)), BC.grid_mesh(), world0=BC.world(1.0, (0.0, 100.0, 0.0)), camera=True)
    return Scene(*BC.refit_scene(1, 300), camera=True)


@pytest.mark.parametrize("mesh,name", [("soup", k) for k in BC.DEFORMATIONS] + [("grid", k) for k in BC.GRID_DEFORMATIONS])
def test_refit_into_a_deformed_shape_and_back(built, mesh, name):
    s = _deformation_scene(mesh)
    try:
        s.ctx.set_refit_policy(NO_REBUILD, 16)
        v0 = s.meshes[1][0]
        built_ = {1: s.arrays(1)}
        f, min_hits = (BC.GRID_DEFORMATIONS if mesh == "grid" else BC.DEFORMATIONS)[name]
        s.frame({1: f(v0)})
        hits = check_after_refit(s, built_, {1: s.meshes[1][0]}, "%s, %s" % (mesh, name), min_hits)[1]
        if name == "folded":      # coincident triangles give equal t and the lower primitive id wins, on both sides (compared above)
            assert (hits["prim"][hits["valid"] & (hits["inst"] == 1)] < BC.FOLDED_GRID_WINNERS).all()
        s.frame({1: v0})
        same_bits(s.arrays(1)[0], built_[1][0], "%s, back from %s" % (mesh, name))
        assert s.ctx.refit_stats(1)["rebuilds"] == 0
    finally:
        s.close()


# ---- c. staging --------------------------------------------------------------------------------------------------------------------
class DeviceShapes:
    """Shapes handed over with rtggx_refit_as_device from ONE torch buffer written on a side stream and overwritten right behind the call."""

    def __init__(self):
        import torch
        self.torch, self.stream, self.keep = torch, torch.cuda.Stream(), []

    def refit(self, scene, slot, v):
        t = self.torch
        src = t.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
        with t.cuda.stream(self.stream):
            buf = t.empty_like(src)
            buf.copy_(src, non_blocking=True)
            scene.ctx.refit_as_device(slot, buf.data_ptr(), buf.shape[0], self.stream.cuda_stream)
            buf.fill_(float("nan"))
        self.keep += [src, buf]
        scene.set_shape(slot, v)

    def done(self):
        self.torch.cuda.synchronize()
        self.keep = []


def test_a_staged_shape_waits_for_a_frame_and_the_newest_wins(built):
    s = Scene(*BC.refit_scene(1, 300), camera=True)
    try:
        s.ctx.set_refit_policy(NO_REBUILD, 16)
        v0 = s.meshes[1][0]
        built_ = {1: s.arrays(1)}
        a, b, c = BC.size_shapes(v0)
        rays = BC.refit_rays(v0, s.worlds[1], seed=300)
        seen = s.ctx.trace_rays(rays)
        s.ctx.refit_as(1, a)                                       # no frame: nothing that readback / trace_rays see changes
        same_bits(s.arrays(1)[0], built_[1][0], "refit_as without a frame")
        again = s.ctx.trace_rays(rays)
        for k in seen:
            assert np.array_equal(seen[k].view(np.uint8), again[k].view(np.uint8)), "refit_as without a frame: %s" % k
        s.ctx.refit_as(1, b)                                       # two calls between frames: the second shape wins
        s.set_shape(1, b)
        s.frame()
        check_after_refit(s, built_, {1: b}, "two refit_as between frames")
        dev = DeviceShapes()
        s.ctx.refit_as(1, a); dev.refit(s, 1, c)                   # host then device: the device shape wins
        s.frame(); dev.done()
        check_after_refit(s, built_, {1: c}, "refit_as, then refit_as_device")
        dev.refit(s, 1, b); s.ctx.refit_as(1, a); s.set_shape(1, a)      # device then host: the host shape wins
        s.frame(); dev.done()
        check_after_refit(s, built_, {1: a}, "refit_as_device, then refit_as")
        assert s.ctx.refit_stats(1)["refits"] == 3
    finally:
        s.close()


@pytest.mark.parametrize("n", [1, 2, 300])
def test_shapes_from_device_memory_equal_shapes_from_the_host(built, n):
    sh, sd = Scene(*BC.refit_scene(1, n), camera=True), Scene(*BC.refit_scene(1, n), camera=True)
    try:
        dev = DeviceShapes()
        built_ = {1: sh.arrays(1)}
        for s in (sh, sd):
            s.ctx.set_refit_policy(NO_REBUILD, 16)
        for f, shape in enumerate(BC.size_shapes(sh.meshes[1][0])):
            sh.frame({1: shape})
            dev.refit(sd, 1, shape); sd.frame(); dev.done()
            same_bits(sd.arrays(1)[0], sh.arrays(1)[0], "%d triangles, shape %d from device memory" % (n, f))
            check_after_refit(sd, built_, {1: shape}, "%d triangles, shape %d from device memory" % (n, f))
    finally:
        sh.close(); sd.close()


def test_both_slots_deform_in_the_same_frames(built):
    """issuePendingRefits refits both on one stream; triBox / nodeBox belong to each mesh's topology, the node arrays to the input set."""
    s = Scene(*BC.refit_scene(0, 97), camera=True)      # 97 triangles in the ground slot, 300 in the model's
    try:
        s.ctx.set_refit_policy(NO_REBUILD, 16)
        built_ = {k: s.arrays(k) for k in (0, 1)}
        shapes = [BC.size_shapes(s.meshes[k][0]) for k in (0, 1)]
        for f, (i, j) in enumerate(((0, 2), (1, None), (None, None), (2, 0), (None, 1))):      # together, one alone, none, together, the other alone
            new = {k: shapes[k][x] for k, x in ((0, i), (1, j)) if x is not None}
            s.frame(new)
            check_after_refit(s, built_, {k: s.meshes[k][0] for k in (0, 1)}, "both slots, frame %d" % f)
    finally:
        s.close()


# ---- d. cost -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 257, 3073])
def test_cost_ratio_against_the_model(built, n):
    """The cost is sampled on every fourth refit: after five consecutive frames of ONE shape the reported figure belongs to it.  Each of
    the two sums (treeCostKernel, fp32) has n - 1 non-negative terms of three rounded operations each, added in an order that is not
    fixed: relative error of the ratio at most 2 (n + 3) 2^-24.  One triangle has no node: the ratio is reported as 1."""
    s = Scene(*BC.refit_scene(1, n), camera=True)
    try:
        s.ctx.set_refit_policy(NO_REBUILD, 16)
        built_nodes = s.arrays(1)[0][0]
        shape = BC.size_shapes(s.meshes[1][0])[1]
        for _ in range(5):
            s.frame({1: shape})
        got = s.ctx.refit_stats(1)["cost_ratio"]
        if n == 1:
            assert got == 1.0
            return
        want = refit_ref.tree_cost(s.arrays(1)[0][0], s.ctx.bvh_root(1)) / refit_ref.tree_cost(built_nodes, s.ctx.bvh_root(1))
        print("cost ratio of %d triangles: device %.9g, model %.9g, relative difference %.3g, bound %.3g" % (n, got, want, abs(got - want) / want, 2 * (n + 3) * 2.0 ** -24))
        assert abs(got - want) <= 2 * (n + 3) * 2.0 ** -24 * want
    finally:
        s.close()


# ---- e. the rebuild beside the frames --------------------------------------------------------------------------------------------
def blown_up(v0):
    """Every vertex somewhere in a box five times the mesh's: nothing the build's topology put together is together any more (the model's
    cost on the build's topology: 18 x the build's for 2 triangles, 61 x for 33, 368 x for 1026)."""
    return BC.scrambled(BC.scaled(5.0)(v0), seed=5)


def mild(shape, f):
    return BC.jitter(shape, seed=100 + f, amount=0.01)


class Rebuild:
    """A scene whose model is blown up at frame 0 and then keeps changing mildly, one frame at a time."""

    def __init__(self, n, spf):
        self.s = Scene(*BC.refit_scene(1, n), camera=True)
        self.s.ctx.set_refit_policy(1.5, spf)
        self.n, self.spf, self.f, self.sent = n, spf, 0, []
        self.limit = -(-REBUILD_STEPS // spf) + 16              # frames within which the rebuild must have ended
        self.big = blown_up(self.s.meshes[1][0])
        arrays, root = self.s.arrays(1)
        if n > 1:      # the model's cost of the new shape on the build's topology: far beyond the threshold, whatever fp32 summation does
            grown = refit_ref.tree_cost(refit_ref.refit_expect(*arrays, root, self.big, self.s.meshes[1][1])[0]) / refit_ref.tree_cost(arrays[0])
            assert grown >= 3 * 1.5, "the blown-up shape costs only %.2f x the build's" % grown

    def frame(self, new_shape=True, check=True):
        """One frame (with the next shape, or none); (ii) and (iii) on it; returns the rebuilds counted so far."""
        shape = None
        if new_shape:
            shape = self.big if self.f == 0 else mild(self.big, self.f)
            self.sent.append(shape)
        self.s.frame({1: shape} if shape is not None else None)
        self.f += 1
        if check:
            structure_and_hits(self.s, (1,), "%d triangles, %d steps per frame, frame %d" % (self.n, self.spf, self.f - 1))
        return self.s.ctx.refit_stats(1)["rebuilds"]

    def until_swapped(self, new_shape=lambda f: True):
        """Frames until the new topology has taken over: the number of the frame that swapped."""
        while self.f < self.limit + 5:
            if self.frame(new_shape(self.f)) >= 1:
                return self.f - 1
        raise AssertionError("%d triangles, %d steps per frame: no rebuild within %d frames: %s" % (self.n, self.spf, self.f, self.s.ctx.refit_stats(1)))


@pytest.mark.parametrize("spf", [1, 4096])
@pytest.mark.parametrize("n", [2, 33, 1026])
def test_rebuild_beside_the_frames(built, n, spf):
    """One launch per frame (the rebuild spans tens of frames while new shapes keep arriving) and all launches at once.  The cost that
    asks for the rebuild is an atomicAdd over several workgroups: no exact frame number is asserted, only the order of events."""
    r = Rebuild(n, spf)
    s = r.s
    try:
        before = s.arrays(1)
        swap = r.until_swapped()
        # the cost is sampled on every fourth refit and read by the next refit_as, whose frame starts the rebuild: up to five frames
        assert swap <= r.limit
        if spf == 1:
            assert swap > 8 + 5, "42 launches, one per frame, ended within %d frames" % swap
        # the new topology: the 4-wide collapse is the surface-area rule's for the shape the rebuild started from -- one of those sent
        # while it cannot have started later (all its launches were out before the swap)
        arrays, root = s.arrays(1)
        last_start = swap - -(-REBUILD_STEPS // spf)
        errors = []
        for k in reversed(range(last_start + 1)):
            snap = refit_ref.refit_expect(*arrays, root, r.sent[k], s.meshes[1][1])
            try:
                bvh_checks.bvh4_check(snap[0], snap[2], root, built_shape=True, weights=s.ctx.collapse_weights())
                break
            except AssertionError as e:
                errors.append("shape of frame %d: %s" % (k, e))
        else:
            raise AssertionError("the rebuilt collapse is the rule's for none of the shapes it can have started from: " + "; ".join(errors[:3]))
        if n > 2:
            assert not np.array_equal(arrays[0][:, 12:14], before[0][0][:, 12:14]), "the rebuild kept the old topology"
        for _ in range(6):
            assert r.frame() == 1
        assert s.ctx.refit_stats(1)["cost_ratio"] < 1.5
    finally:
        s.close()


@pytest.mark.parametrize("spf", [1, 4096])
def test_deformation_stops_at_the_swap(built, spf):
    """No new shape from the frame that swaps on: three of the input sets hold an older shape and are refitted on the new topology, the
    fourth is current in its vertices, is NOT refitted and keeps the old topology's arrays -- traced with the new topology's root, depth
    and stack.  Every set's arrays must be a valid tree of the current vertices.  (The frame that swaps is learned from a first context
    that keeps deforming; the second replays its frames.)"""
    first = Rebuild(33, spf)
    try:
        swap = first.until_swapped()
    finally:
        first.s.close()
    r = Rebuild(33, spf)
    try:
        assert r.until_swapped(lambda f: f < swap) >= swap, "the replay swapped while shapes were still arriving"
        for _ in range(4):
            assert r.frame(new_shape=False) == 1
    finally:
        r.s.close()


@pytest.mark.parametrize("how", ["build_as", "set_mesh"])
def test_build_while_a_rebuild_is_in_flight(built, how):
    """abandonRebuild: rtggx_build_as, or rtggx_set_mesh with another triangle count and then rtggx_build_as, halfway between the start
    of a one-launch-per-frame rebuild and its swap (both learned from a first context; the rebuild spans 42 frames)."""
    first = Rebuild(33, 1)
    try:
        swap = first.until_swapped()
    finally:
        first.s.close()
    r = Rebuild(33, 1)
    s = r.s
    try:
        for _ in range(swap - REBUILD_STEPS // 2):
            assert r.frame(check=False) == 0
        if how == "set_mesh":
            s.meshes[1] = BC.mesh_from_tris(BC.soup(20, seed=21))
            s.ctx.set_mesh(1, *s.meshes[1]); s.o.set_mesh(1, *s.meshes[1])
            r.big = s.meshes[1][0]
        s.ctx.build_as()
        s.ctx.set_refit_policy(NO_REBUILD, 1)
        structure_and_hits(s, (1,), how + " in mid-rebuild", refitted=())      # built from the newest shape, which the current set holds
        for _ in range(6):
            assert r.frame() == 0
    finally:
        s.close()


def test_a_mesh_built_collapsed_is_rebuilt_once_it_has_grown(built):
    """A growth animation that starts collapsed: 300 triangles built with all vertices on one axis-aligned line (equal Morton codes on
    two axes, a summed half-area of exactly 0), then refitted into an ordinary soup.  Hits are right on every frame, because a refit
    always is; and the tree, made for a line, must be rebuilt: a build of cost 0 with a current cost above 0 asks for it."""
    mesh0, mesh1, w0, w1 = BC.refit_scene(1, 300)
    v0 = mesh1[0]
    # (built_shape: the surface-area rule divides by the root's half-area, 0 here: it says nothing about this build's collapse)
    s = Scene(mesh0, (BC.to_line(v0), mesh1[1]), w0, w1, camera=True, built_shape=(True, False))
    try:
        s.ctx.set_refit_policy(1.5, 16)
        assert refit_ref.tree_cost(s.arrays(1)[0][0]) == 0.0
        for f in range(24):
            s.frame({1: BC.jitter(v0, seed=200 + f, amount=0.01)})
            structure_and_hits(s, (1,), "grown from a line, frame %d" % f)
        st = s.ctx.refit_stats(1)
        assert st["rebuilds"] >= 1, "never rebuilt: %s" % st
        assert st["cost_ratio"] < 1.5, st
    finally:
        s.close()
