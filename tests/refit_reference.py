"""numpy float32 restatement of rt_blas_refit (no GPU, no library).

Given the rt_blas_export arrays of a BLAS as it was BEFORE the refit (uint32 views: nodes (nn, 32), triangle
records (n, 12)) and the new vertices and the build's indices, refit() returns the arrays the refit must leave:

  * triangle record i (leaf order) = v0, v1 - v0, v2 - v0 of triangle tris[i].prim's new positions; prim and the
    two padding words copied;
  * a leaf slot's box = min / max of the triangle's three vertices, + 0.0 (a -0.0 bound becomes +0.0);
  * an internal slot's box = the exact min / max union of that child node's valid slots;
  * child refs, count, first_inner, inner_mask, entry_base and the empty slots (kEmptyChild, their boxes) copied.

Nodes are walked in descending index: the build numbers them breadth first, so every internal child's index
exceeds its parent's (asserted) and a child is finished before its parent reads it.

Node words (Bvh4Node, 128 B): lox[4] hix[4] loy[4] hiy[4] loz[4] hiz[4] | child[4] | count first_inner
inner_mask entry_base.
"""
import numpy as np

EMPTY = -(2 ** 31) + 1  # kEmptyChild
LO = (0, 8, 16)         # word of lo.x / lo.y / lo.z of slot 0; hi is 4 further, slot k is k further
CHILD = 24


def positions_of(vertices, indices, prim):
    """The three float32 positions (each (m, 3)) of triangles `prim`."""
    pos = np.ascontiguousarray(np.asarray(vertices, np.float32)[:, :3])
    prim = np.asarray(prim, np.int64)
    if indices is None:
        i0, i1, i2 = 3 * prim, 3 * prim + 1, 3 * prim + 2
    else:
        idx = np.asarray(indices, np.int64).ravel()
        i0, i1, i2 = idx[3 * prim], idx[3 * prim + 1], idx[3 * prim + 2]
    return pos[i0], pos[i1], pos[i2]


def refit_tris(tris_u32, vertices, indices):
    out = np.array(tris_u32, dtype=np.uint32).reshape(-1, 12).copy()
    a, b, c = positions_of(vertices, indices, out[:, 3])
    f = out.view(np.float32)
    f[:, 0:3] = a
    f[:, 4:7] = b - a
    f[:, 8:11] = c - a
    return out


def refit(nodes_u32, tris_u32, vertices, indices):
    """-> (nodes, tris) as uint32 arrays of the exported shapes."""
    tris = refit_tris(tris_u32, vertices, indices)
    nodes = np.array(nodes_u32, dtype=np.uint32).reshape(-1, 32).copy()
    nn = nodes.shape[0]
    f = nodes.view(np.float32)
    child = nodes[:, CHILD:CHILD + 4].view(np.int32)
    a, b, c = positions_of(vertices, indices, tris[:, 3])
    zero = np.float32(0.0)
    leaf_lo = np.minimum(np.minimum(a, b), c) + zero
    leaf_hi = np.maximum(np.maximum(a, b), c) + zero
    # per node and slot, for the unions: empty slots never win a min / max
    lo = np.full((nn, 4, 3), np.inf, np.float32)
    hi = np.full((nn, 4, 3), -np.inf, np.float32)
    leaf = (child < 0) & (child != EMPTY)
    slot = ~child[leaf]
    assert slot.size == 0 or (slot.min() >= 0 and slot.max() < tris.shape[0]), "leaf ref outside the BLAS"
    lo[leaf], hi[leaf] = leaf_lo[slot], leaf_hi[slot]
    for i in range(nn - 1, -1, -1):
        for k in range(4):
            ck = int(child[i, k])
            if ck >= 0:
                assert i < ck < nn, f"node {i} slot {k}: internal child {ck} does not follow its parent"
                lo[i, k], hi[i, k] = lo[ck].min(axis=0), hi[ck].max(axis=0)
    valid = child != EMPTY
    for ax in range(3):
        for k in range(4):
            v = valid[:, k]
            f[v, LO[ax] + k] = lo[v, k, ax]
            f[v, LO[ax] + 4 + k] = hi[v, k, ax]
    return nodes, tris


def root_bounds(nodes_u32):
    """(lo, hi) of node 0's valid slots: the BLAS bounds after the refit."""
    nodes = np.asarray(nodes_u32, np.uint32).reshape(-1, 32)
    f = nodes.view(np.float32)
    valid = nodes[0, CHILD:CHILD + 4].view(np.int32) != EMPTY
    lo = np.array([f[0, LO[ax]:LO[ax] + 4][valid].min() for ax in range(3)], np.float32)
    hi = np.array([f[0, LO[ax] + 4:LO[ax] + 8][valid].max() for ax in range(3)], np.float32)
    return lo, hi
