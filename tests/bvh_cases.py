"""The pure-numpy part of what the BVH tests share (tests/test_gpu_bvh_meshes.py, tests/test_gpu_bvh_refit.py and the host test of
the refit model, tests/test_refit_ref_host.py): instance transforms and the frame constants that carry them, synthetic meshes, ray
sets, and the deformations a refit is tested with.  Nothing here needs a GPU or the built library."""
import numpy as np

W = H = 64               # the contexts of the BVH tests


# ---- instance transforms and constants -------------------------------------------------------------------------------------------
def world(scale=1.0, translate=(0.0, 0.0, 0.0), rot_y90=False):
    """Row-vector 4x4 (p' = p M, as XMMATRIX): uniform scale, optional quarter turn about y, translation -- all exact in fp32."""
    m = np.eye(4, dtype=np.float32) * np.float32(scale)
    m[3, 3] = 1.0
    if rot_y90:
        m[:3, :3] = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], np.float32) * np.float32(scale)
    m[3, :3] = translate
    return m


def frame_constants(world0, world1, base=None):
    """The 768-byte RtggxFrameConstants with only Worlds[2] set (float4x3, XMStoreFloat3x4: f[j * 4 + i] = M[i][j], j < 3); `base`: the
    768 bytes everything else is taken from (an ordinary camera's constants for the tests that run the visibility pass)."""
    fc = np.zeros(192, np.float32) if base is None else np.frombuffer(bytes(base), np.float32).copy()
    for k, w in enumerate((world0, world1)):
        fc[64 + 12 * k:76 + 12 * k] = np.asarray(w, np.float32)[:, :3].T.reshape(-1)
    return fc.tobytes()


# ---- meshes ----------------------------------------------------------------------------------------------------------------------
def mesh_from_tris(tris):
    """[n, 3, 3] triangles -> (verts [3n, 6] with a +y normal, idx [3n])."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    v = np.zeros((tris.shape[0] * 3, 6), np.float32)
    v[:, :3] = tris.reshape(-1, 3)
    v[:, 4] = 1.0
    return v, np.arange(v.shape[0], dtype=np.uint32)


def soup(n, seed, extent=1.0, size=None):
    rng = np.random.default_rng(seed)
    size = size if size is not None else extent * 1.5 * max(n, 1) ** (-1.0 / 3.0)
    c = rng.uniform(-extent, extent, (n, 1, 3))
    return (c + rng.normal(0.0, size, (n, 3, 3))).astype(np.float32)


def grid_mesh(q=128, step=0.125):
    """Flat grid of q x q quads in y = 0, two triangles each, shared vertices: zero Morton extent along y, equal boxes per quad."""
    k = np.arange(q + 1, dtype=np.float32)
    x, z = np.meshgrid((k - q / 2) * np.float32(step), (k - q / 2) * np.float32(step), indexing="ij")
    v = np.zeros(((q + 1) ** 2, 6), np.float32)
    v[:, 0], v[:, 2], v[:, 4] = x.reshape(-1), z.reshape(-1), 1.0
    a = (np.arange(q)[:, None] * (q + 1) + np.arange(q)[None, :]).reshape(-1)
    idx = np.stack([a, a + 1, a + q + 1, a + 1, a + q + 2, a + q + 1], 1).reshape(-1).astype(np.uint32)
    return v, idx


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def rays_through_box(lo, hi, n, seed, tmin=0.0, tmax=1e30):
    """Origins on a sphere around the box, targets uniform inside it; direction = target - origin (t = 1 at the target)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, r = 0.5 * (lo + hi), max(float(np.linalg.norm(hi - lo)), 1e-3)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    org = c + 1.5 * r * d
    tgt = rng.uniform(lo, hi, (n, 3))
    return np.concatenate([org, tgt - org, np.full((n, 1), tmin), np.full((n, 1), tmax)], 1).astype(np.float32)


def world_box(verts, world_matrix):
    """World-space box of a mesh's vertices (the instance transforms here are scale, quarter turn and translation: corners suffice)."""
    v = np.asarray(verts)[:, :3].astype(np.float64)
    corners = np.array([[x, y, z] for x in (v[:, 0].min(), v[:, 0].max()) for y in (v[:, 1].min(), v[:, 1].max())
                        for z in (v[:, 2].min(), v[:, 2].max())])
    p = np.concatenate([corners, np.ones((8, 1))], 1) @ np.asarray(world_matrix).astype(np.float64)
    return p[:, :3].min(axis=0), p[:, :3].max(axis=0)


def refit_rays(verts, world_matrix, seed, n=1500):
    """The ray set a refitted mesh is traced with: n rays through its new world-space box, and n / 2 aimed at vertices of the new
    shape from outside.

    A mesh that has collapsed into a point or onto an axis-aligned line (two or three axes without extent) consists of zero-area
    triangles only.  A ray that passes such a triangle within rounding has no defined answer: a watertight edge-function test sees
    three edge values that are rounding noise and reports a hit whenever they happen to agree in sign, and a box of no extent may or
    may not be culled first -- brute force and ANY tree can differ there, and neither is wrong.  So for these shapes the rays are
    chosen to have exact answers: the box is widened by 0.5 along the axes without extent before rays are sent through it (they pass
    the collapsed mesh at a clear distance), and the aimed rays lie exactly in a coordinate plane that contains the point or line
    (origin and vertex share that coordinate bit for bit, the direction's component is 0): every triangle's edge values are then
    exactly 0, a definite miss, while the ray still walks down the zero-extent boxes to the leaves it is aimed at.  This needs the
    instance transform to keep that coordinate exact (scale 1, a translation of few bits), which is asserted."""
    m = np.asarray(world_matrix).astype(np.float64)
    v = np.asarray(verts)[:, :3].astype(np.float64)
    rng = np.random.default_rng(seed + 7919)
    pick = v[rng.integers(0, len(v), n // 2)]
    thin = v.max(axis=0) == v.min(axis=0)
    if thin.sum() < 2:
        lo, hi = world_box(verts, world_matrix)
        through = rays_through_box(lo, hi, n, seed)
        tgt = np.concatenate([pick, np.ones((n // 2, 1))], 1) @ m
        aimed = through[:n // 2].copy()
        aimed[:, 3:6] = (tgt[:, :3] - aimed[:, :3].astype(np.float64)).astype(np.float32)
        return np.concatenate([through, aimed])
    wide = np.array(verts, np.float64)
    wide = np.concatenate([wide, wide])
    wide[:len(v), :3] -= 0.5 * thin; wide[len(v):, :3] += 0.5 * thin
    through = rays_through_box(*world_box(wide, world_matrix), n, seed)
    axis = int(np.nonzero(thin)[0][0])                  # the coordinate origin and vertex share
    off = rng.normal(size=(n // 2, 3)); off[:, axis] = 0.0
    off *= 3.0 / np.linalg.norm(off, axis=1, keepdims=True)
    org = np.concatenate([pick + off, np.ones((n // 2, 1))], 1) @ m
    aimed = np.concatenate([org[:, :3], -off @ m[:3, :3], np.zeros((n // 2, 1)), np.full((n // 2, 1), 1e30)], 1).astype(np.float32)
    inv = np.linalg.inv(m)
    back_o = np.concatenate([aimed[:, :3].astype(np.float64), np.ones((n // 2, 1))], 1) @ inv
    back_d = aimed[:, 3:6].astype(np.float64) @ inv[:3, :3]
    assert (back_o[:, axis] == v[0, axis]).all() and (back_d[:, axis] == 0.0).all(), "the aimed rays do not lie exactly in the plane of the collapsed mesh"
    return np.concatenate([through, aimed])


# ---- deformations ----------------------------------------------------------------------------------------------------------------
# Each takes the vertices [nv, 6] of the build's shape and returns new ones (normals untouched: the trees do not read them).
def _moved(v0, pos):
    v = np.array(v0, np.float32)
    v[:, :3] = np.asarray(pos, np.float32)
    return v


def jitter(v0, seed=1, amount=0.02):
    return _moved(v0, v0[:, :3] + np.random.default_rng(seed).normal(0.0, amount, (len(v0), 3)))


def scrambled(v0, seed=2):
    """Every vertex to a fresh random position in the mesh's box (in a unit box where that is flat): the topology fits nothing."""
    lo, hi = v0[:, :3].min(axis=0).astype(np.float64), v0[:, :3].max(axis=0).astype(np.float64)
    flat = hi - lo < 1e-3
    return _moved(v0, np.random.default_rng(seed).uniform(np.where(flat, lo - 0.5, lo), np.where(flat, hi + 0.5, hi), (len(v0), 3)))


def to_point(v0):
    return _moved(v0, np.broadcast_to(np.array([0.25, -0.125, 0.5], np.float32), (len(v0), 3)))


def to_line(v0):
    """Onto the axis-aligned line y = 0.25, z = -0.5 (x kept): boxes of zero extent on two axes, zero half-area."""
    p = v0[:, :3].copy()
    p[:, 1], p[:, 2] = 0.25, -0.5
    return _moved(v0, p)


def to_plane(v0):
    """Into the plane y = 0, written as -0.0."""
    p = v0[:, :3].copy()
    p[:, 1] = -0.0
    return _moved(v0, p)


def scaled(factor):
    def f(v0):
        return _moved(v0, v0[:, :3] * np.float32(factor))
    f.__name__ = "scaled_%g" % factor
    return f


def folded_grid(v0):
    """The grid's half x > 0 moved by exactly half the grid's width: every quad of it then lies on a quad of the other half with the
    same three vertices per triangle, bit for bit (the one column of quads at x = 0 is stretched across).  Every hit meets two or more
    triangles at the same t."""
    p = v0[:, :3].copy()
    half = p[:, 0].max()
    p[:, 0] = np.where(p[:, 0] > 0, p[:, 0] - half, p[:, 0])
    return _moved(v0, p)


# Every triangle of the moved half beyond the stretched column has a twin of equal vertices and lower id in the other half: equal t bit
# for bit, so the lower id wins and no primitive from FOLDED_GRID_WINNERS on (q = 128: the first q / 2 + 1 columns of quads) is ever hit.
FOLDED_GRID_WINNERS = 2 * 128 * (128 // 2 + 1)


# name -> (deformation, the least number of rays of refit_rays that must hit; 0 where the shape has no area to hit)
DEFORMATIONS = {"jitter": (jitter, 1), "scrambled": (scrambled, 1), "point": (to_point, 0), "line": (to_line, 0), "plane": (to_plane, 1),
                "times_1e6": (scaled(1e6), 1), "times_1e-6": (scaled(1e-6), 1)}
GRID_DEFORMATIONS = dict(DEFORMATIONS, folded=(folded_grid, 1))


# ---- the cases of the refit tests: the same meshes, transforms and ray sets on the host (the model alone) and on the GPU -----------
SLOT1_SIZES = [1, 2, 3, 5, 17, 33, 257, 1025, 1026, 2049, 3073]      # 1026: 1025 nodes, the first tree whose root is a level-1 treelet
SLOT0_SIZES = [1, 2, 13, 17, 97]                                     # 97 fills the ground's table of 16


def refit_scene(slot, n):
    """(mesh0, mesh1, world0, world1) of the case "a soup of n triangles in `slot` deforms"."""
    if slot == 1:
        return (mesh_from_tris(soup(12, seed=100)), mesh_from_tris(soup(n, seed=n)),
                world(4.0, (0.0, -6.0, 0.0)), world(1.0, (0.25, 0.5, -0.125), rot_y90=(n % 2 == 1)))
    return (mesh_from_tris(soup(n, seed=1000 + n)), mesh_from_tris(soup(300, seed=7)), world(2.0, (0.5, 0.0, 0.0)), world(1.0, (0.0, 0.0, 0.5)))


def size_shapes(v0):
    """The three shapes a mesh of the size cases is refitted through: a mild jitter, a sheared and bent one, a strong jitter."""
    bent = v0[:, :3].astype(np.float64) * [1.5, 0.75, 1.25]
    bent[:, 0] += 0.5 * np.sin(2.0 * v0[:, 1]); bent[:, 1] += 0.25 * v0[:, 2]
    return [jitter(v0, seed=11, amount=0.05), _moved(v0, bent), jitter(v0, seed=13, amount=0.2)]
