"""An exact model of a BVH refit (csrc/lbvh.hip refitLbvh: refitTris, refitTreelets, emitNodes, emitNodes4, emitTop) and of the cost
it reports (treeCostKernel), in plain numpy.  A refit is fully determined by the arrays before it and the new vertices, and it has no
rounding: leaf records get the new vertices, every box is a min / max of fp32 values, every reference stays.  So what it must leave is
known bit for bit -- except the sign of a zero box coordinate (fminf(-0.0f, 0.0f) may return either), which is why boxes are compared
as float values and everything else as bit patterns (same_arrays).

Record layouts (include/rtggx.h, csrc/rtggx_device.h), in 32-bit words:
  leaf triangle, 16 words: v0 v1 v2 (9 floats), the primitive id at word 9 (pad0[0]) and at word 12
  binary node, 16 words:   child-0 box min / max, child-1 box min / max, child references at words 12, 13 (>= 0: node, < 0: ~leaf slot)
  4-wide node, 32 words:   minx[4] miny[4] minz[4] maxx[4] maxy[4] maxz[4] ref[4] level pad[3]; ref == EMPTY: no entry; a slot of the
                           sparse array that is no 4-wide node is all zero
  top table:               4-wide nodes in breadth-first order from the root, a reference to a node inside the table reads TOP_FLAG | rank"""
import numpy as np

EMPTY = 0x7FFFFFFF
TOP_FLAG = 0x40000000


def _levels(child, root):
    levels, frontier = [], np.array([root], np.int64)
    while frontier.size:
        levels.append(frontier)
        c = child[frontier].reshape(-1)
        frontier = c[c >= 0].astype(np.int64)
        assert len(levels) <= len(child) + 1, "cycle"
    return levels


def refit_expect(nodes, tris, nodes4, top, root, verts, idx):
    """The four arrays of one input set (BUF_BVH_NODES*, BUF_BVH_TRIS*, BUF_BVH4_NODES*, BUF_BVH4_TOP*, as uint32) that a refit of this
    tree to `verts` ([nv, 6]; `idx`: the mesh's index buffer) must leave.  nodes4 / top may be empty (a tree without a collapse: the
    oracle's)."""
    nodes = np.array(nodes, np.uint32).reshape(-1, 16)
    tris = np.array(tris, np.uint32).reshape(-1, 16)
    nodes4 = np.array(nodes4, np.uint32).reshape(-1, 32)
    top = np.array(top, np.uint32).reshape(-1, 32)
    n = len(tris)
    # leaf records: the same slot order and primitive ids, the new vertices bit for bit
    prims = tris[:, 12].astype(np.int64)
    pos = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 6)[:, :3])
    tri_idx = np.asarray(idx, np.int64).reshape(-1, 3)
    tv = pos[tri_idx[prims]]                                  # [n, 3 vertices, 3]
    tris[:, :9] = tv.reshape(n, 9).view(np.uint32)
    if n < 2:
        return nodes, tris, nodes4, top
    leaf_box = np.concatenate([tv.min(axis=1), tv.max(axis=1)], 1)      # [n, 6] fp32: min / max are exact
    # binary nodes: the same child references, each child box the min / max over everything below it, bottom-up level by level
    child = nodes[:, 12:14].view(np.int32)
    node_box = np.zeros((len(nodes), 6), np.float32)                    # a node's own box: the union of its two child boxes
    f = nodes.view(np.float32)
    for level in reversed(_levels(child, root)):
        side = []
        for s, off in ((0, 0), (1, 6)):
            c = child[level, s].astype(np.int64)
            box = np.where((c < 0)[:, None], leaf_box[np.where(c < 0, ~c, 0)], node_box[np.where(c < 0, 0, c)])
            f[level, off:off + 6] = box
            side.append(box)
        node_box[level, :3] = np.minimum(side[0][:, :3], side[1][:, :3])
        node_box[level, 3:] = np.maximum(side[0][:, 3:], side[1][:, 3:])
    # 4-wide nodes: the same references and level in every used slot, each entry's box the binary tree's box of what it names
    if nodes4.size:
        used = np.nonzero(nodes4.any(axis=1))[0]
        f4 = nodes4.view(np.float32)
        ref = nodes4[:, 24:28].view(np.int32)
        for e in range(4):
            r = ref[used, e].astype(np.int64)
            empty = r == EMPTY
            box = np.where((r < 0)[:, None], leaf_box[np.where(r < 0, ~r, 0)], node_box[np.where((r < 0) | empty, 0, r)])
            box = np.where(empty[:, None], np.array([np.inf] * 3 + [-np.inf] * 3, np.float32), box)
            for k in range(6):
                f4[used, 4 * k + e] = box[:, k]
    # top table: the same references, the boxes of the 4-wide nodes they stand for
    if top.size:
        node_of = {0: int(root)}
        for k in range(len(top)):
            node = node_of[k]
            r = top[k, 24:28].view(np.int32)
            for e in range(4):
                if r[e] >= 0 and r[e] != EMPTY and (r[e] & TOP_FLAG):
                    node_of[int(r[e]) & ~TOP_FLAG] = int(nodes4[node, 24 + e])
            top[k, :24] = nodes4[node, :24]
    return nodes, tris, nodes4, top


def tree_cost(nodes, root=None):
    """The sum, in float64, over all n - 1 nodes of the half-area (ex ey + ey ez) + ez ex of the node's own box -- the union of its two
    child boxes, the root's included: what treeCostKernel adds up in fp32."""
    f = np.asarray(nodes, np.uint32).reshape(-1, 16).view(np.float32).astype(np.float64)
    lo, hi = np.minimum(f[:, 0:3], f[:, 6:9]), np.maximum(f[:, 3:6], f[:, 9:12])
    e = hi - lo
    return float(((e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]).sum())


def same_arrays(got, want, label):
    """(nodes, tris, nodes4, top) against (nodes, tris, nodes4, top): references, primitive ids, levels and leaf vertices as bit
    patterns, boxes as float values (-0.0 equals +0.0)."""
    names = ("binary nodes", "leaf triangles", "4-wide nodes", "top table")
    for name, g, w in zip(names, got, want):
        width = 32 if name in ("4-wide nodes", "top table") else 16
        g, w = np.asarray(g, np.uint32).reshape(-1, width), np.asarray(w, np.uint32).reshape(-1, width)
        assert g.shape == w.shape, "%s: %s has %d records, expected %d" % (label, name, len(g), len(w))
        boxes = 0 if name == "leaf triangles" else 12 if name == "binary nodes" else 24
        bad = np.nonzero((g[:, boxes:] != w[:, boxes:]).any(axis=1))[0]
        assert bad.size == 0, "%s: %s: %d records differ in their words (references, ids, vertices), first %d: %s, expected %s" % (
            label, name, bad.size, bad[0], g[bad[0], boxes:].tolist(), w[bad[0], boxes:].tolist())
        bad = np.nonzero((g[:, :boxes].view(np.float32) != w[:, :boxes].view(np.float32)).any(axis=1))[0]
        assert bad.size == 0, "%s: %s: %d records differ in their boxes, first %d: %s, expected %s" % (
            label, name, bad.size, bad[0], g[bad[0], :boxes].view(np.float32).tolist(), w[bad[0], :boxes].view(np.float32).tolist())
