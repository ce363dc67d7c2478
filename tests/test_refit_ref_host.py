"""The refit model (tests/refit_ref.py) on the host, against the oracle: the oracle builds a tree of its own in the device's layout;
refit_expect of that tree for a new shape must be a valid tree of the new shape (bvh_checks.bvh_check: leaf vertices bit for bit, every
box exactly the min / max of what is below it), and the oracle walking the model's arrays must find what its brute-force loop over the
moved triangles finds, bit for bit -- on the meshes, shapes and ray sets tests/test_gpu_bvh_refit.py uses, whose min_hits are asserted
here as well: that the rays reach the deformed mesh at all is a property of the reference alone."""
import numpy as np
import pytest

import bvh_cases as BC
import bvh_checks
import refit_ref
from oracle import oracle as O

KEYS = ("inst", "prim", "t", "b1", "b2")


def _oracle(slot, n):
    mesh0, mesh1, w0, w1 = BC.refit_scene(slot, n)
    o = O.Oracle(BC.W, BC.H)
    o.set_mesh(0, *mesh0); o.set_mesh(1, *mesh1)
    o.build_as()
    o.set_frame_constants(BC.frame_constants(w0, w1)); o.update_as()
    return o, (mesh0, mesh1), (w0, w1)


def _check_shape(o, trees, meshes, worlds, slot, v, min_hits, label):
    nodes, tris, root = trees[slot]
    idx = meshes[slot][1]
    empty = np.zeros((0, 32), np.uint32)
    m_nodes, m_tris, _, _ = refit_ref.refit_expect(nodes, tris, empty, empty, root, v, idx)
    bvh_checks.bvh_check(m_nodes, m_tris, root, idx.size // 3, v, idx)
    o.set_mesh(slot, v, idx)
    o.set_bvh(slot, m_nodes, m_tris, root)
    o.set_bvh(1 - slot, *trees[1 - slot])
    rays = BC.refit_rays(v, worlds[slot], seed=idx.size // 3)
    b, w = o.trace_rays(rays, brute=True), o.trace_rays(rays)
    assert np.array_equal(b["valid"], w["valid"]), "%s: a hit on one side only" % label
    for k in KEYS:
        assert np.array_equal(b[k][b["valid"]].view(np.uint32), w[k][b["valid"]].view(np.uint32)), "%s: %s differs" % (label, k)
    hits = int((b["valid"] & (b["inst"] == slot)).sum())
    assert hits >= min_hits, "%s: %d of %d rays hit the deformed mesh" % (label, hits, len(rays))


@pytest.mark.parametrize("slot,n", [(1, n) for n in BC.SLOT1_SIZES if n <= 300] + [(0, n) for n in BC.SLOT0_SIZES])
def test_model_of_the_size_cases(slot, n):
    o, meshes, worlds = _oracle(slot, n)
    try:
        trees = [o.get_bvh(s) for s in (0, 1)]
        v0 = meshes[slot][0]
        for k, v in enumerate(BC.size_shapes(v0) + [v0]):
            _check_shape(o, trees, meshes, worlds, slot, v, 1, "slot %d, %d triangles, shape %d" % (slot, n, k))
    finally:
        o.close()


@pytest.mark.parametrize("n", [1, 2, 3, 17, 300])
@pytest.mark.parametrize("name", list(BC.DEFORMATIONS))
def test_model_of_the_deformations(name, n):
    o, meshes, worlds = _oracle(1, n)
    try:
        trees = [o.get_bvh(s) for s in (0, 1)]
        f, min_hits = BC.DEFORMATIONS[name]
        _check_shape(o, trees, meshes, worlds, 1, f(meshes[1][0]), min_hits, "%d triangles, %s" % (n, name))
    finally:
        o.close()


@pytest.mark.parametrize("name", list(BC.GRID_DEFORMATIONS))
def test_ray_sets_of_the_deformed_grid_reach_it(name):
    """(The 32 768-triangle grid is too large for a CPU tree walk in a quick test; brute force over a slice of its ray set is not.)"""
    v0, idx = BC.grid_mesh()
    f, min_hits = BC.GRID_DEFORMATIONS[name]
    v = f(v0)
    o = O.Oracle(BC.W, BC.H)
    try:
        o.set_mesh(0, *BC.mesh_from_tris(BC.soup(12, seed=100))); o.set_mesh(1, v, idx)
        o.set_frame_constants(BC.frame_constants(BC.world(1.0, (0.0, 100.0, 0.0)), BC.world())); o.update_as()
        rays = BC.refit_rays(v, BC.world(), seed=idx.size // 3)[:200]
        b = o.trace_rays(rays, brute=True)
        assert int((b["valid"] & (b["inst"] == 1)).sum()) >= min(min_hits, 1)
        if name == "folded":
            assert (b["prim"][b["valid"] & (b["inst"] == 1)] < BC.FOLDED_GRID_WINNERS).all()
    finally:
        o.close()


@pytest.mark.parametrize("n", [1, 2, 3, 17, 300])
def test_refit_to_the_unchanged_vertices_changes_nothing(n):
    o, meshes, _ = _oracle(1, n)
    try:
        nodes, tris, root = o.get_bvh(1)
        empty = np.zeros((0, 32), np.uint32)
        got = refit_ref.refit_expect(nodes, tris, empty, empty, root, *meshes[1])
        refit_ref.same_arrays(got, (nodes, tris, empty, empty), "%d triangles" % n)
        assert np.array_equal(got[1], tris)
    finally:
        o.close()


def test_tree_cost_of_a_known_tree():
    """Two triangles, one node: the cost is the half-area of the union of the two child boxes."""
    node = np.zeros((1, 16), np.float32)
    node[0, 0:6] = [0, 0, 0, 1, 2, 3]; node[0, 6:12] = [-1, 0, 1, 0.5, 1, 4]
    ex, ey, ez = 2.0, 2.0, 4.0
    assert refit_ref.tree_cost(node.view(np.uint32), 0) == ex * ey + ey * ez + ez * ex
