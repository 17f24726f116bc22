"""Axis-aligned scenes and lattice rays for holding the BVH walk to brute force (test helper, plain numpy).

The random-scene tests aim rays in general position at random soups, where the slab test's rounding never decides
anything. Here everything sits on a lattice: quads and boxes with corners on multiples of 1/4, rays that start on
the same lattice, run parallel to an axis or inside an axis plane, or carry one direction component so small that
o / d is huge. Those are the rays that lie exactly in the face planes of the BVH's boxes, and the ones whose slab
distances lose every digit of the plane offset.

Scenes (each under one identity instance, `ONE`, and under the three-instance set `THREE`):
  grid(n, axis, h)   2 n^2 triangles: n x n quads of side 1/2 in the plane coordinate[axis] = h, centred on the origin
  boxes(m)           12 m triangles: m boxes with corners on multiples of 1/2 (coincident faces happen)
  flat_floor(verts)  the library's ground plane (the caller passes rt_plane_vertices: this module imports neither
                     the device library nor torch); its box has zero thickness
Ray classes (`rays`), N_RAYS rays each, tmin 0, tmax 1e5, no non-finite values, no zero-length directions:
  axis      one component +-1, the others +-0 (both signs of zero); origins on the 1/4 lattice, 0.0 and -0.0 included
  planar    one component +-0, that origin coordinate on the lattice; the rest in general position
  grazing   that component one of +-1e-7, +-1e-12, +-1e-22, +-1e-30, +-1e-38; aimed at lattice points 5 - 500 away
  far       the same from 1e3 - 1e4 away
  generic   a third each of the first three classes with continuous origins (the control: clean before and after)
Every ray is aimed at a point of the scene (a lattice point of some triangle's box, moved into a random instance of
the set), so a good part of each class hits.

`compare` tolerates ties: axis-aligned scenes have coincident and edge-sharing triangles, so several primitives sit
at the minimum t. It compares the hit flag and the bits of t alone, which is what a wrongly culled triangle changes.
A walk that culls the t = +0 hit of one instance and keeps the t = -0 hit of another shows up as `nearer` (the bits
differ, the value is not larger): that is what every `nearer` ray of these scenes was before the cull was looked at,
a lost triangle and no flaw of brute force.
"""
import numpy as np

N_RAYS = 6000
TMAX = 100000.0
TINY = (1e-7, 1e-12, 1e-22, 1e-30, 1e-38)
CLASSES = ("axis", "planar", "grazing", "far", "generic")

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
ONE = (IDENTITY,)
THREE = (IDENTITY,
         np.array([1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, 0], np.float32),     # translation (0.5, 0, 0)
         np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 2, 3], np.float32))      # scale (1, -1, 2), translation (0, 0, 3)
INSTANCE_SETS = {"one": ONE, "three": THREE}


def _soup(p, normal=(0.0, 1.0, 0.0)):
    """p: (ntri, 3, 3) positions -> (3 ntri, 6) float32 vertices (non-indexed)."""
    v = np.zeros((p.shape[0] * 3, 6), np.float32)
    v[:, :3] = np.asarray(p, np.float64).reshape(-1, 3)
    v[:, 3:] = normal
    return v


def grid(n, axis, h):
    """n x n quads of side 1/2 in the plane coordinate[axis] = h, two triangles each, vertices duplicated per cell
    (every interior edge is a positional twin)."""
    u, w = [k for k in range(3) if k != axis]
    tris = []
    for i in range(n):
        for j in range(n):
            c = np.full((4, 3), float(h))
            c[:, u] = np.array([i, i + 1, i + 1, i]) * 0.5 - n * 0.25
            c[:, w] = np.array([j, j, j + 1, j + 1]) * 0.5 - n * 0.25
            tris += [c[[0, 1, 2]], c[[0, 2, 3]]]
    nrm = [0.0, 0.0, 0.0]
    nrm[axis] = 1.0
    return _soup(np.asarray(tris), nrm)


_BOX_QUADS = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))


def boxes(m, seed=40):
    """m axis-aligned boxes, corners on multiples of 1/2 in x, z in [-4, 4] and y in [-1, 3.5]; 12 triangles each."""
    rng = np.random.default_rng(seed)
    tris = []
    for _ in range(m):
        size = rng.integers(1, 4, size=3) * 0.5
        lo = np.array([rng.integers(-8, 8 - int(size[0] * 2) + 1), 0, rng.integers(-8, 8 - int(size[2] * 2) + 1)]) * 0.5
        lo[1] = -1.0 + rng.integers(0, 7) * 0.5
        hi = lo + size
        c = np.array([[(lo, hi)[(k >> 2) & 1][0], (lo, hi)[(k >> 1) & 1][1], (lo, hi)[k & 1][2]] for k in range(8)])
        for q in _BOX_QUADS:
            tris += [c[[q[0], q[1], q[2]]], c[[q[0], q[2], q[3]]]]
    return _soup(np.asarray(tris))


def flat_floor(plane_vertices):
    return np.ascontiguousarray(plane_vertices, np.float32).reshape(-1, 6)


def scene_table(plane_vertices):
    """name -> (vertices, triangle count the issue states); built once per test module."""
    t = {}
    for n in (9, 16):
        for axis, h in ((0, 1.5), (1, 0.0), (2, -0.75)):
            t[f"grid{n}{'xyz'[axis]}"] = grid(n, axis, h)
    t["boxes40"] = boxes(40)
    t["floor"] = flat_floor(plane_vertices)
    assert t["grid9x"].shape[0] == 3 * 162 and t["grid16y"].shape[0] == 3 * 512 and t["boxes40"].shape[0] == 3 * 480
    return t


def _apply(x, p):
    m = np.asarray(x, np.float64).reshape(3, 4)
    return p @ m[:, :3].T + m[:, 3]


def _targets(rng, verts, xforms, n, continuous):
    """Points of the scene: a lattice point (multiples of 1/4; continuous: any point) of a random triangle's box,
    or one of its vertices, moved into a random instance of the set (half of them into the first, the identity).
    The transforms keep the 1/4 lattice."""
    tri = verts[:, :3].astype(np.float64).reshape(-1, 3, 3)
    k = rng.integers(0, tri.shape[0], size=n)
    lo, hi = tri[k].min(axis=1), tri[k].max(axis=1)
    if continuous:  # off the lattice on every axis, the flat axis of an axis-aligned triangle too
        p = lo + rng.random((n, 3)) * (hi - lo) + rng.uniform(-0.2, 0.2, size=(n, 3))
    else:
        steps = np.round((hi - lo) * 4.0)
        p = lo + np.floor(rng.random((n, 3)) * (steps + 1.0)) * 0.25
        at_vertex = rng.random(n) < 0.25
        p[at_vertex] = tri[k[at_vertex], rng.integers(0, 3, size=int(at_vertex.sum()))]
    which = np.where(rng.random(n) < 0.5, 0, rng.integers(0, len(xforms), size=n))
    out = np.empty_like(p)
    for i, x in enumerate(xforms):
        out[which == i] = _apply(x, p[which == i])
    return out


def _signed_zero(rng, shape):
    return np.where(rng.random(shape) < 0.5, 0.0, -0.0)


def _class(rng, verts, xforms, cls, n, continuous):
    """(origins float64, directions float64, special (n, 3) bool: the components that are zero or tiny)."""
    p = _targets(rng, verts, xforms, n, continuous)
    a = rng.integers(0, 3, size=n)
    rows = np.arange(n)
    special = np.zeros((n, 3), bool)
    if cls == "axis":
        d = _signed_zero(rng, (n, 3))
        s = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        d[rows, a] = s
        back = rng.integers(0, 41, size=n) * 0.25  # 0: the origin lies on the target itself
        if continuous:
            back = back + rng.random(n)
        o = p.copy()
        o[rows, a] -= s * back
        special[:] = True
        special[rows, a] = False
        return o, d, special
    d = rng.normal(size=(n, 3))
    d[rows, a] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    special[rows, a] = True
    if cls == "planar":
        d[rows, a] = _signed_zero(rng, n)
        dist = rng.uniform(0.5, 12.0, size=n)
    else:
        d[rows, a] = rng.choice(TINY, size=n) * np.where(rng.random(n) < 0.5, 1.0, -1.0)
        lo, hi = (5.0, 500.0) if cls == "grazing" else (1e3, 1e4)
        dist = np.exp(rng.uniform(np.log(lo), np.log(hi), size=n))
    return p - dist[:, None] * d, d, special


def rays(verts, xforms, cls, seed=0, n=N_RAYS):
    """-> (rays (n, 8) float32 in rt_trace_rays' layout, special (n, 3) bool)."""
    rng = np.random.default_rng([seed, CLASSES.index(cls)])
    if cls == "generic":
        parts = [_class(rng, verts, xforms, c, n // 3, True) for c in ("axis", "planar", "grazing")]
        o, d, special = (np.concatenate([q[i] for q in parts]) for i in range(3))
    else:
        o, d, special = _class(rng, verts, xforms, cls, n, False)
    r = np.zeros((o.shape[0], 8), np.float32)
    r[:, :3], r[:, 4:7], r[:, 7] = o, d, TMAX
    if cls != "generic":  # both signs of an origin coordinate that is zero
        z = (r[:, :3] == 0.0) & (rng.random((o.shape[0], 3)) < 0.5)
        r[:, :3][z] = -0.0
    assert np.isfinite(r).all() and (np.abs(r[:, 4:7]).max(axis=1) > 0.5).all()
    return r, special


def compare(walk, brute, any_hit=False):
    """walk, brute: (n, 4) uint32 hit records (t bits, instance, primitive, flag). Counts of rays where
    lost: brute force hits, the walk misses; extra: the walk hits, brute force misses; farther / nearer: both hit and
    the walk's t is larger / smaller (closest hit only: an any-hit walk may stop at any accepted triangle).
    hits: brute force's hit count."""
    w, b = walk[:, 3] != 0, brute[:, 3] != 0
    out = {"hits": int(b.sum()), "lost": int((b & ~w).sum()), "extra": int((w & ~b).sum()), "farther": 0, "nearer": 0}
    if not any_hit:
        both = w & b
        tw, tb = walk[:, 0].copy().view(np.float32), brute[:, 0].copy().view(np.float32)
        differ = both & (walk[:, 0] != brute[:, 0])
        out["farther"] = int((differ & (tw > tb)).sum())
        out["nearer"] = int((differ & ~(tw > tb)).sum())
    return out


def total(counts):
    """Sum of compare()'s results over several modes."""
    return {k: sum(c[k] for c in counts) for k in ("lost", "farther", "nearer", "extra")}


def node_planes(nodes):
    """The min-face and max-face plane coordinates of every box of exported 4-wide nodes ((nn, 32) uint32: lox[4],
    hix[4], loy[4], hiy[4], loz[4], hiz[4], child[4], ...), per axis: ([lo_x, lo_y, lo_z], [hi_x, hi_y, hi_z])."""
    f = np.ascontiguousarray(nodes[:, :24]).view(np.float32).reshape(-1, 6, 4)
    used = np.isfinite(f).all(axis=1)  # empty slots hold +inf boxes
    return ([np.unique(f[:, 2 * k][used]) for k in range(3)], [np.unique(f[:, 2 * k + 1][used]) for k in range(3)])


def in_face_planes(nodes, r, special):
    """(rays lying in a min-face plane, rays lying in a max-face plane) of some box of `nodes`: an origin coordinate
    equal to the plane's, on an axis whose direction component is zero or tiny (special)."""
    lo, hi = node_planes(nodes)
    in_lo = np.zeros(r.shape[0], bool)
    in_hi = np.zeros(r.shape[0], bool)
    for k in range(3):
        in_lo |= special[:, k] & np.isin(r[:, k], lo[k])
        in_hi |= special[:, k] & np.isin(r[:, k], hi[k])
    return int(in_lo.sum()), int(in_hi.sum())


# The frame case: the boxes on the floor under one light so far above the origin that every shadow ray is vertical to
# within |d.x|, |d.z| ~ 1e-7 |P| (the hit points of camera rays are no lattice points, so exactly vertical shadow rays
# cannot come out of a frame; the `axis` class holds those).
FRAME_LIGHT = ((1.0, 1.0, 1.0), (0.0, 1.0e7, 0.0), 1.0)
FRAME_CAMERA = ((7.0, 6.0, 9.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
FRAME_SIZE = (64, 40)

# What the walk loses against brute force, per (scene, instance set, class): strict xfails, with the counts measured on
# the oracle's per-ray walk (closest hit without culling, then the sums over the four modes as lost / farther /
# nearer). tests/test_walk_bruteforce_host.py says what they are and what was tried. A case that starts to pass fails
# its strict xfail: take it out of the table then. Every class but `generic` is here for every scene; of the control
# class one case is, a ray in general position between two instances' coincident faces (the same rounding of o / d).
RESIDUAL = {
    ("grid9x", "one", "axis"): "lost 316, farther 0, nearer 0 of 2009 closest hits (four modes: 948 / 0 / 0)",
    ("grid9x", "one", "planar"): "lost 398, farther 0, nearer 0 of 3862 closest hits (four modes: 1194 / 0 / 0)",
    ("grid9x", "one", "grazing"): "lost 610, farther 0, nearer 0 of 3668 closest hits (four modes: 1830 / 0 / 0)",
    ("grid9x", "one", "far"): "lost 550, farther 0, nearer 0 of 3610 closest hits (four modes: 1650 / 0 / 0)",
    ("grid9x", "three", "axis"): "lost 253, farther 19, nearer 0 of 1948 closest hits (four modes: 993 / 19 / 0)",
    ("grid9x", "three", "planar"): "lost 267, farther 59, nearer 0 of 3920 closest hits (four modes: 1080 / 88 / 0)",
    ("grid9x", "three", "grazing"): "lost 453, farther 64, nearer 0 of 4118 closest hits (four modes: 1757 / 108 / 0)",
    ("grid9x", "three", "far"): "lost 409, farther 79, nearer 0 of 4098 closest hits (four modes: 1671 / 128 / 0)",
    ("grid9y", "one", "axis"): "lost 304, farther 0, nearer 0 of 1951 closest hits (four modes: 912 / 0 / 0)",
    ("grid9y", "one", "planar"): "lost 369, farther 0, nearer 0 of 3891 closest hits (four modes: 1107 / 0 / 0)",
    ("grid9y", "one", "grazing"): "lost 1145, farther 0, nearer 0 of 4702 closest hits (four modes: 3435 / 0 / 0)",
    ("grid9y", "one", "far"): "lost 1149, farther 0, nearer 0 of 4695 closest hits (four modes: 3447 / 0 / 0)",
    ("grid9y", "three", "axis"): "lost 175, farther 0, nearer 3 of 2034 closest hits (four modes: 525 / 0 / 6)",
    ("grid9y", "three", "planar"): "lost 207, farther 0, nearer 0 of 3910 closest hits (four modes: 621 / 0 / 0)",
    ("grid9y", "three", "grazing"): "lost 979, farther 0, nearer 0 of 5215 closest hits (four modes: 2937 / 0 / 0)",
    ("grid9y", "three", "far"): "lost 994, farther 0, nearer 0 of 5194 closest hits (four modes: 2982 / 0 / 0)",
    ("grid9z", "one", "axis"): "lost 339, farther 0, nearer 0 of 2040 closest hits (four modes: 1017 / 0 / 0)",
    ("grid9z", "one", "planar"): "lost 387, farther 0, nearer 0 of 3847 closest hits (four modes: 1161 / 0 / 0)",
    ("grid9z", "one", "grazing"): "lost 508, farther 0, nearer 0 of 3872 closest hits (four modes: 1524 / 0 / 0)",
    ("grid9z", "one", "far"): "lost 476, farther 0, nearer 0 of 3817 closest hits (four modes: 1428 / 0 / 0)",
    ("grid9z", "three", "axis"): "lost 256, farther 35, nearer 0 of 2018 closest hits (four modes: 1055 / 35 / 0)",
    ("grid9z", "three", "planar"): "lost 306, farther 36, nearer 0 of 3994 closest hits (four modes: 1080 / 36 / 0)",
    ("grid9z", "three", "grazing"): "lost 423, farther 53, nearer 0 of 4060 closest hits (four modes: 1429 / 53 / 0)",
    ("grid9z", "three", "far"): "lost 426, farther 46, nearer 0 of 3967 closest hits (four modes: 1427 / 46 / 0)",
    ("grid16x", "one", "axis"): "lost 88, farther 0, nearer 0 of 2009 closest hits (four modes: 264 / 0 / 0)",
    ("grid16x", "one", "planar"): "lost 137, farther 0, nearer 0 of 3916 closest hits (four modes: 411 / 0 / 0)",
    ("grid16x", "one", "grazing"): "lost 442, farther 0, nearer 0 of 3782 closest hits (four modes: 1326 / 0 / 0)",
    ("grid16x", "one", "far"): "lost 409, farther 0, nearer 0 of 3690 closest hits (four modes: 1227 / 0 / 0)",
    ("grid16x", "three", "axis"): "lost 68, farther 21, nearer 0 of 1948 closest hits (four modes: 333 / 21 / 0)",
    ("grid16x", "three", "planar"): "lost 67, farther 41, nearer 0 of 3950 closest hits (four modes: 376 / 62 / 0)",
    ("grid16x", "three", "grazing"): "lost 313, farther 77, nearer 0 of 4233 closest hits (four modes: 1311 / 137 / 0)",
    ("grid16x", "three", "far"): "lost 288, farther 99, nearer 0 of 4155 closest hits (four modes: 1239 / 171 / 0)",
    ("grid16y", "one", "axis"): "lost 98, farther 0, nearer 0 of 1951 closest hits (four modes: 294 / 0 / 0)",
    ("grid16y", "one", "planar"): "lost 119, farther 0, nearer 0 of 3941 closest hits (four modes: 357 / 0 / 0)",
    ("grid16y", "one", "grazing"): "lost 997, farther 0, nearer 0 of 4801 closest hits (four modes: 2991 / 0 / 0)",
    ("grid16y", "one", "far"): "lost 1034, farther 0, nearer 0 of 4825 closest hits (four modes: 3102 / 0 / 0)",
    ("grid16y", "three", "axis"): "lost 24, farther 0, nearer 0 of 2034 closest hits (four modes: 72 / 0 / 0)",
    ("grid16y", "three", "planar"): "lost 42, farther 0, nearer 0 of 3945 closest hits (four modes: 126 / 0 / 0)",
    ("grid16y", "three", "grazing"): "lost 902, farther 0, nearer 0 of 5270 closest hits (four modes: 2706 / 0 / 0)",
    ("grid16y", "three", "far"): "lost 896, farther 0, nearer 0 of 5175 closest hits (four modes: 2688 / 0 / 0)",
    ("grid16z", "one", "axis"): "lost 99, farther 0, nearer 0 of 2040 closest hits (four modes: 297 / 0 / 0)",
    ("grid16z", "one", "planar"): "lost 125, farther 0, nearer 0 of 3872 closest hits (four modes: 375 / 0 / 0)",
    ("grid16z", "one", "grazing"): "lost 351, farther 0, nearer 0 of 3970 closest hits (four modes: 1053 / 0 / 0)",
    ("grid16z", "one", "far"): "lost 335, farther 0, nearer 0 of 3910 closest hits (four modes: 1005 / 0 / 0)",
    ("grid16z", "three", "axis"): "lost 54, farther 35, nearer 0 of 2018 closest hits (four modes: 287 / 35 / 0)",
    ("grid16z", "three", "planar"): "lost 91, farther 36, nearer 0 of 4031 closest hits (four modes: 365 / 36 / 0)",
    ("grid16z", "three", "grazing"): "lost 283, farther 70, nearer 0 of 4178 closest hits (four modes: 996 / 70 / 0)",
    ("grid16z", "three", "far"): "lost 286, farther 74, nearer 0 of 4059 closest hits (four modes: 996 / 74 / 0)",
    ("boxes40", "one", "axis"): "lost 1351, farther 1341, nearer 0 of 6000 closest hits (four modes: 5490 / 4103 / 0)",
    ("boxes40", "one", "planar"): "lost 703, farther 818, nearer 0 of 5875 closest hits (four modes: 2688 / 2325 / 0)",
    ("boxes40", "one", "grazing"): "lost 462, farther 551, nearer 0 of 5557 closest hits (four modes: 1709 / 1440 / 0)",
    ("boxes40", "one", "far"): "lost 428, farther 527, nearer 0 of 5530 closest hits (four modes: 1572 / 1371 / 0)",
    ("boxes40", "three", "axis"): "lost 641, farther 1468, nearer 0 of 6000 closest hits (four modes: 2645 / 4611 / 0)",
    ("boxes40", "three", "planar"): "lost 375, farther 951, nearer 0 of 5944 closest hits (four modes: 1448 / 2758 / 0)",
    ("boxes40", "three", "grazing"): "lost 266, farther 616, nearer 0 of 5793 closest hits (four modes: 1005 / 1696 / 0)",
    ("boxes40", "three", "far"): "lost 267, farther 602, nearer 0 of 5792 closest hits (four modes: 1007 / 1610 / 0)",
    ("boxes40", "three", "generic"): "lost 0, farther 1, nearer 0 of 5518 closest hits (four modes: 0 / 2 / 0)",
    ("floor", "one", "axis"): "lost 304, farther 0, nearer 0 of 1951 closest hits (four modes: 912 / 0 / 0)",
    ("floor", "one", "planar"): "lost 435, farther 0, nearer 0 of 3759 closest hits (four modes: 1305 / 0 / 0)",
    ("floor", "one", "grazing"): "lost 166, farther 0, nearer 0 of 4356 closest hits (four modes: 498 / 0 / 0)",
    ("floor", "one", "far"): "lost 108, farther 0, nearer 0 of 3755 closest hits (four modes: 324 / 0 / 0)",
    ("floor", "three", "axis"): "lost 252, farther 60, nearer 0 of 2034 closest hits (four modes: 756 / 120 / 0)",
    ("floor", "three", "planar"): "lost 329, farther 82, nearer 0 of 3826 closest hits (four modes: 987 / 164 / 0)",
    ("floor", "three", "grazing"): "lost 121, farther 33, nearer 0 of 4614 closest hits (four modes: 363 / 66 / 0)",
    ("floor", "three", "far"): "lost 98, farther 27, nearer 0 of 4043 closest hits (four modes: 294 / 54 / 0)",
}

# The same for the watertight test against rt_host_trace_triangles where that alone fails (tests/
# test_gpu_walk_bruteforce.py; measured on the device, the only place the watertight walk runs): control-class rays
# under the three-instance set whose hit lies on two instances' coincident triangles, answered by the farther one. Only
# `farther` occurs, never `nearer`, `lost` or `extra`, which is the cull's signature and not a reference's. Checked on
# the CPU for the two grids: of the control rays whose two nearest instances' watertight t (rt_host_trace_triangles)
# lie within 1e-6 of each other, exactly one per grid is a ray for which the oracle's walk over the nearer instance
# alone, given the other instance's t as its tmax (the walk's tbest at that point), drops the box while brute force
# with that tmax hits: the rounding of o / d against a competing t, as in boxes40 / three / generic above. The same
# replay finds none of the floor's 7 rays (736 candidates), so for the floor the mechanism is still only supposed.
RESIDUAL_WATERTIGHT = {
    ("grid9x", "three", "generic"): "watertight: farther 1 of 3083 closest hits (6 of 48 runs differ)",
    ("grid16x", "three", "generic"): "watertight: farther 1 of 3188 closest hits (6 of 48 runs differ)",
    ("floor", "three", "generic"): "watertight: farther 7 of 3255 closest hits, 1 of 1644 with back and 6 of 1611 with "
                                   "front culling (18 of 48 runs differ)",
}
