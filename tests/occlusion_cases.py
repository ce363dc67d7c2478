"""Meshes of the occlusion tests (tests/test_gpu_occlusion.py, tests/occlusion_forced_child.py).  Pure numpy, like bvh_cases.py."""
import numpy as np

from bvh_cases import mesh_from_tris, soup

SMALL0 = mesh_from_tris(soup(12, seed=100))      # the ground slot's mesh where a case is about the model's


def telescope(copies=100, s=0.9):
    """Copies of one triangle, each s times the size of the one before and moved toward -z by half the room that leaves: every copy's box
    lies strictly inside the box of every larger copy, so the tree is a caterpillar `copies` levels deep and a traversal stack of 16
    entries spills (tests/test_gpu_bvh_meshes.py builds the same mesh and shows that it does).  Returns the triangles, smallest first, and
    the z of the smallest copy's centre."""
    base = np.array([[-1.0, -1.0, -1.0], [1.0, -1.0, 0.0], [0.0, 1.0, 1.0]])
    tris, zc = [], 0.0
    for k in range(copies):
        tris.append(base * s ** k + np.array([0.0, 0.0, zc]))
        zc -= 0.5 * s ** k * (1.0 - s)
    return np.array(tris[::-1], np.float32), np.float32(zc + 0.5 * s ** (copies - 1) * (1.0 - s))


LONG_W, LONG_H = 1024, 512      # 8192 bins of 64 slots: the context's bins hold 524 288 rays per launch


def long_list_context():
    """A context whose bins hold the long lists in one launch, an oracle with the same two overlapping soups for the brute force, and 262 144
    rays aimed into a box twice the model's: the oracle's brute force finds 69 % of 2000 such rays occluded (97 % of those aimed into the
    model's own box: too few of the rays that have to walk every subtree they enter).  The caller closes both."""
    import bvh_cases
    from oracle import oracle as O
    from raytracedggx_amd import capi
    meshes = (mesh_from_tris(soup(97, seed=1097)), mesh_from_tris(soup(5000, seed=21)))
    worlds = (bvh_cases.world(2.0, (0.5, 0.0, 0.0)), bvh_cases.world(1.0, (0.0, 0.0, 0.5)))
    ctx, o = capi.Context(LONG_W, LONG_H), O.Oracle(bvh_cases.W, bvh_cases.H)
    try:
        for slot, (v, i) in enumerate(meshes):
            ctx.set_mesh(slot, v, i); o.set_mesh(slot, v, i)
        ctx.build_as()
        fc = bvh_cases.frame_constants(*worlds)
        ctx.update_frame(fc); ctx.update_as()
        o.set_frame_constants(fc); o.update_as()
        lo, hi = (np.asarray(x, np.float64) for x in bvh_cases.world_box(meshes[1][0], worlds[1]))
        return ctx, o, bvh_cases.rays_through_box(1.5 * lo - 0.5 * hi, 1.5 * hi - 0.5 * lo, 262144, seed=23)
    except Exception:
        ctx.close(); o.close()
        raise


def check_long_list(ctx, o, rays, n):
    """The first n rays: trace_occlusion against the closest-hit kernel's valid (which the existing tests pin to the oracle) on every ray, against
    brute force on 4096 of them spread over the list, and against itself on a second call."""
    rays = rays[:n]
    occ = ctx.trace_occlusion(rays)
    valid = ctx.trace_rays(rays)["valid"]
    bad = np.nonzero(occ != valid)[0]
    assert bad.size == 0, "%d rays: %d differ from the closest-hit kernel, first ray %d" % (n, bad.size, bad[0])
    pick = np.arange(4096) * (n // 4096)
    b = o.trace_rays(rays[pick], brute=True)["valid"]
    np.testing.assert_array_equal(occ[pick], b, err_msg="%d rays: the sample against brute force" % n)
    assert 0.05 * n < occ.sum() < 0.95 * n, "%d of %d rays occluded" % (occ.sum(), n)
    np.testing.assert_array_equal(ctx.trace_occlusion(rays), occ, err_msg="a repeated call")
