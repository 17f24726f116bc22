"""rt_blas_refit without a GPU: the two entry points exist and reject a null context, and the numpy restatement the
GPU tests compare against (tests/refit_reference.py) is itself checked on hand-written trees whose boxes come from
an independent formulation (the min / max over ALL vertices below a slot, not a union of child slots)."""
import numpy as np
import pytest

import realtimeraytracing_gradproject_amd as rt

import refit_reference as ref

E = ref.EMPTY

# Hand-written BVH4 topologies in breadth-first order; a slot is ("n", node), ("t", leaf slot) or None (empty).
# 5 triangles, two levels: the root holds one internal child, one triangle and two empty slots.
TREE5 = [
    [("n", 1), ("t", 4), None, None],
    [("t", 0), ("t", 1), ("t", 2), ("t", 3)],
]
# 17 triangles: internal children in the lowest slots (as the BLAS build leaves them), leaves beside them, empty
# slots at two levels, and a third level so that a union of unions is exercised.
TREE17 = [
    [("n", 1), ("n", 2), ("n", 3), ("t", 16)],
    [("n", 4), ("t", 0), ("t", 1), None],
    [("t", 6), ("t", 7), ("t", 8), ("t", 9)],
    [("n", 5), ("t", 10), ("t", 11), None],
    [("t", 2), ("t", 3), ("t", 4), ("t", 5)],
    [("t", 12), ("t", 13), ("t", 14), ("t", 15)],
]


def mesh(ntri, seed):
    """ntri triangles, non-indexed; triangle 0 lies in the plane x = -0.0 and one more coordinate is -0.0."""
    rng = np.random.default_rng(seed)
    v = np.zeros((ntri * 3, 6), np.float32)
    v[:, :3] = rng.uniform(-2.0, 2.0, size=(ntri * 3, 3)).astype(np.float32)
    v[:, 4] = 1.0
    v[0:3, 0] = np.float32(-0.0)
    v[5, 2] = np.float32(-0.0)
    return v


def leaves_below(tree, node):
    out = []
    for s in tree[node]:
        if s is None:
            continue
        out += leaves_below(tree, s[1]) if s[0] == "n" else [s[1]]
    return out


def write_arrays(tree, verts, perm):
    """The export arrays of `tree` over `verts`: leaf slot s holds triangle perm[s]; a slot's box is the min / max of
    every vertex of every triangle below it (+ 0.0, the canonical zero)."""
    ntri = len(perm)
    pos = verts[:, :3].reshape(ntri, 3, 3)
    tris = np.zeros((ntri, 12), np.uint32)
    tf = tris.view(np.float32)
    for s, p in enumerate(perm):
        a, b, c = pos[p]
        tf[s, 0:3], tf[s, 4:7], tf[s, 8:11] = a, b - a, c - a
        tris[s, 3] = p
    nodes = np.zeros((len(tree), 32), np.uint32)
    nf, ni = nodes.view(np.float32), nodes.view(np.int32)
    for i, slots in enumerate(tree):
        inner = [s[1] for s in slots if s is not None and s[0] == "n"]
        mask = 0
        for k, s in enumerate(slots):
            if s is None:
                ni[i, 24 + k] = E
                nf[i, [0 + k, 8 + k, 16 + k, 4 + k, 12 + k, 20 + k]] = np.inf  # lo = hi = +inf
                continue
            if s[0] == "n":
                below, ni[i, 24 + k], mask = leaves_below(tree, s[1]), s[1], mask | (1 << k)
            else:
                below, ni[i, 24 + k] = [s[1]], ~s[1]
            pts = np.concatenate([pos[perm[t]] for t in below])
            lo, hi = pts.min(axis=0) + np.float32(0.0), pts.max(axis=0) + np.float32(0.0)
            for ax in range(3):
                nf[i, 8 * ax + k], nf[i, 8 * ax + 4 + k] = lo[ax], hi[ax]
        nodes[i, 28] = sum(s is not None for s in slots)
        ni[i, 29] = inner[0] if inner else 0
        nodes[i, 30] = mask
        nodes[i, 31] = (int(ni[i, 29]) << 8) | (mask << 4)
    return nodes, tris


CASES = [(TREE5, 5, 11), (TREE17, 17, 12)]


def test_entry_points_exist_and_reject_a_null_context():
    assert {"rt_blas_refit", "rt_blas_refit_device"} <= {n for n, _, _ in rt.SIGNATURES}
    v = np.zeros((3, 6), np.float32)
    assert rt.lib.rt_blas_refit(None, 0, v.ctypes.data_as(rt._P), 3, 24) == rt.RT_E_INVALID
    assert rt.lib.rt_blas_refit_device(None, 0, v.ctypes.data_as(rt._P), 3, 24, None) == rt.RT_E_INVALID
    assert rt.lib.rt_api_version() == 4


@pytest.mark.parametrize("tree,ntri,seed", CASES, ids=["5", "17"])
def test_reference_reproduces_a_hand_written_tree(tree, ntri, seed):
    verts = mesh(ntri, seed)
    perm = np.random.default_rng(seed).permutation(ntri)
    assert sorted(leaves_below(tree, 0)) == list(range(ntri))
    nodes, tris = write_arrays(tree, verts, perm)
    assert (nodes[:, 24:28].view(np.int32) == E).any(), "the case needs an empty slot"
    assert (verts[:, :3].view(np.uint32) == 0x80000000).any(), "the case needs a -0.0 coordinate"
    got_n, got_t = ref.refit(nodes, tris, verts, None)
    assert np.array_equal(got_t, tris)
    assert np.array_equal(got_n, nodes), f"words differ at {np.argwhere(got_n != nodes)[:8].tolist()}"


@pytest.mark.parametrize("tree,ntri,seed", CASES, ids=["5", "17"])
def test_reference_on_moved_vertices(tree, ntri, seed):
    verts = mesh(ntri, seed)
    perm = np.random.default_rng(seed).permutation(ntri)
    nodes, tris = write_arrays(tree, verts, perm)
    moved = verts.copy()
    rng = np.random.default_rng(seed + 100)
    moved[3:, :3] += rng.normal(scale=0.7, size=(ntri * 3 - 3, 3)).astype(np.float32)  # triangle 0 stays in x = -0.0
    got_n, got_t = ref.refit(nodes, tris, moved, None)
    want_n, want_t = write_arrays(tree, moved, perm)  # the independent formulation again
    assert np.array_equal(got_t, want_t) and np.array_equal(got_n, want_n)
    assert not np.array_equal(got_n, nodes)
    # topology words and empty slots untouched
    assert np.array_equal(got_n[:, 24:], nodes[:, 24:])
    f, child = got_n.view(np.float32), got_n[:, 24:28].view(np.int32)
    for i in range(got_n.shape[0]):
        for k in range(4):
            c = child[i, k]
            if c == E:
                assert np.isposinf(f[i, [k, 4 + k, 8 + k, 12 + k, 16 + k, 20 + k]]).all()
            elif c >= 0:  # the parent's slot contains every valid slot of the child
                v = child[c] != E
                for ax in range(3):
                    assert f[i, 8 * ax + k] <= f[c, 8 * ax:8 * ax + 4][v].min()
                    assert f[i, 8 * ax + 4 + k] >= f[c, 8 * ax + 4:8 * ax + 8][v].max()
    # triangle 0 (x = -0.0 on all three vertices): its leaf slot's x bounds are +0.0, bit pattern 0
    s0 = int(np.nonzero(perm == 0)[0][0])
    where = np.argwhere(child == ~s0)
    assert where.shape[0] == 1
    i, k = where[0]
    assert got_n[i, 0 + k] == 0 and got_n[i, 4 + k] == 0, "a -0.0 coordinate must give a +0.0 bound"
    assert (got_n[:, :24] != 0x80000000).all(), "no -0.0 anywhere in the boxes"
