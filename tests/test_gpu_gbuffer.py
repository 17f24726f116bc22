"""The G-buffer pass on the GPU (rt_dispatch_gbuffer, Context.dispatch_gbuffer, Context.pick).

Every comparison is bit for bit. hits and uv are checked against the CPU oracle tracing RayGen's own camera rays
(oracle.camera_rays: the frame's exact bits), object against the scene description, normal against
rt_host_shading_normals (pinned to numpy restatements by tests/test_gbuffer_host.py) evaluated on the G-buffer's own
(primitive, u, v), and — for model-group hits — against the RT_SHADE_PRIMARY frame the library renders of the same
scene, whose Lambert term is recomputed from the G-buffer's t and normal in float32.

Shapes: 37 x 21 (neither side a multiple of the 8-pixel tile or the 16-pixel workgroup: partial tiles on both
edges, several workgroups), 1 x 1, and 96 x 64 for the random scenes. Every output tensor is pre-filled with 0xAB
bytes and followed by a guard region, so entries the kernel failed to write, or wrote out of bounds, show.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import realtimeraytracing_gradproject_amd as rt  # noqa: E402
from realtimeraytracing_gradproject_amd import scenes  # noqa: E402

import oracle  # noqa: E402
import gbuffer_reference as ref  # noqa: E402
import random_scenes  # noqa: E402

W, H = 37, 21
PLANES = (("hits", 4), ("uv", 2), ("normal", 4), ("object", 2))
FILL = np.uint32(0xABABABAB)
GUARD = 64  # words after each plane
PACKET, LANE = rt.RT_SCHED_PACKET, rt.RT_SCHED_LANE
MISS = np.uint32(0xFFFFFFFF)
TMAX = np.array([100000.0], np.float32).view(np.uint32)[0]


def away(spec):
    """The scene seen from outside with the camera turned away from it: every pixel a miss."""
    s = scenes.SceneSpec(**{**spec.__dict__})
    s.camera = ((7.0, 5.0, 9.0), (14.0, 12.0, 18.0), (0.0, 1.0, 0.0))
    return s


@functools.lru_cache(maxsize=None)
def spec_of(name, w=W, h=H):
    if name.startswith("RND"):
        return random_scenes.random_scene(int(name[3:]), w, h, max_tris=600, models=False)
    if name == "AWAY":
        return away(scenes.config("C2")).with_size(w, h)
    if name == "CHAIN":
        return chain_scene().with_size(w, h)
    return scenes.config(name).with_size(w, h)


def pixel_rays(spec):
    py, px = np.divmod(np.arange(spec.width * spec.height), spec.width)
    return oracle.camera_rays(spec.camera_buffer(), spec.width, spec.height, px, py)


@functools.lru_cache(maxsize=None)
def oracle_planes(name, w=W, h=H):
    """hits (n, 4), uv (n, 2) as uint32 and object (n, 2) of the full frame, from the oracle and the spec; computed
    once per scene and shared (callers do not modify them)."""
    spec = spec_of(name, w, h)
    hits, uv, _ = oracle.Scene(spec).trace_rays(pixel_rays(spec))
    return hits, uv.view(np.uint32), objects_of(spec, hits)


def objects_of(spec, hits):
    group = np.array([hg for (_, _, _, hg) in spec.instances], np.uint32)
    hit = hits[:, 3] == 1
    obj = np.full((hits.shape[0], 2), MISS, np.uint32)
    obj[hit, 0] = hits[hit, 1]
    obj[hit, 1] = group[hits[hit, 1]]
    return obj


def host_normals(spec, hits, uv):
    """The normal plane rt_host_shading_normals gives for these hit records, instance by instance."""
    out = np.zeros((hits.shape[0], 4), np.float32)
    for k, (m, x, _, hg) in enumerate(spec.instances):
        sel = (hits[:, 3] == 1) & (hits[:, 1] == k)
        if sel.any():
            v, i = spec.meshes[m]
            out[sel] = rt.host_shading_normals(v, i, hits[sel, 2], uv[sel].view(np.float32), hg, x)
    return out.view(np.uint32)


def alloc(w, h, rows=None, planes=("hits", "uv", "normal", "object")):
    """Pre-filled output tensors (on torch's current stream), each followed by its guard region."""
    n = (h if rows is None else len(rows)) * w
    return {name: torch.full((n * words + GUARD,), int(FILL.view(np.int32)), dtype=torch.int32, device="cuda")
            for name, words in PLANES if name in planes}


def launch(c, w, h, bufs, rows=None, stream=None):
    """One G-buffer launch into `bufs` (no synchronisation)."""
    args = {name: t[:t.numel() - GUARD] for name, t in bufs.items()}
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    c.dispatch_gbuffer(w, h, rows=rows, stream=s, **args)


def collect(bufs):
    """-> {plane: (n, words) uint32}; the guard regions must still hold the fill."""
    out = {}
    for name, words in PLANES:
        if name in bufs:
            a = bufs[name].cpu().numpy().view(np.uint32)
            assert (a[-GUARD:] == FILL).all(), f"{name}: the guard region after the plane was written"
            out[name] = a[:-GUARD].reshape(-1, words)
    return out


def gbuffer(c, w, h, rows=None, planes=("hits", "uv", "normal", "object")):
    bufs = alloc(w, h, rows, planes)
    launch(c, w, h, bufs, rows)
    torch.cuda.synchronize()
    return collect(bufs)


def assert_plane(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {got.shape[0]} pixels differ, first {bad[0]}: "
                           f"{got[bad[0]]} vs {want[bad[0]]}")


def check_against_oracle(g, name, w=W, h=H, what=None):
    what = what or name
    hits, uv, obj = oracle_planes(name, w, h)
    assert_plane(g["hits"], hits, f"{what} hits")
    assert_plane(g["uv"], uv, f"{what} uv")
    assert_plane(g["object"], obj, f"{what} object")
    assert_plane(g["normal"], host_normals(spec_of(name, w, h), g["hits"], g["uv"]), f"{what} normal")
    miss = g["hits"][:, 3] == 0
    assert (g["hits"][miss] == [TMAX, MISS, MISS, 0]).all() and (g["uv"][miss] == 0).all()
    assert (g["normal"][miss] == 0).all() and (g["normal"][:, 3] == 0).all() and (g["object"][miss] == MISS).all()
    return int((~miss).sum())


def check_primary_frame(c, spec, g, what):
    """-normal and t of the model-group hits reproduce the library's RT_SHADE_PRIMARY frame under one light."""
    light = spec.lights[0]
    c.set_shading([light], spec.material, rt.RT_SHADE_PRIMARY, 1)
    out8 = torch.zeros((spec.height, spec.width, 4), dtype=torch.uint8, device="cuda")
    out32 = torch.zeros((spec.height, spec.width, 4), dtype=torch.float32, device="cuda")
    c.dispatch(spec.width, spec.height, out8, out32, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    frame = out32.cpu().numpy().reshape(-1, 4)
    model = (g["hits"][:, 3] == 1) & (g["object"][:, 1] == rt.RT_HITGROUP_MODEL)
    rays = pixel_rays(spec)[model]
    want = ref.lambert_primary_f32(g["normal"][model].view(np.float32), g["hits"][model, 0].view(np.float32),
                                   rays[:, 0:3], rays[:, 4:7], light[1])
    got = frame[model]
    for ch in range(3):
        bad = np.nonzero(got[:, ch].view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, f"{what}: PRIMARY frame differs on {bad.size} of {int(model.sum())} model hits"
    return int(model.sum())


# 1, 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [PACKET, LANE], ids=["packet", "lane"])
@pytest.mark.parametrize("name", ["REF", "C2", "C2F", "DEGEN"])
def test_planes_equal_oracle_and_host_normals(name, schedule):
    spec = spec_of(name)
    with rt.Context(0) as c:
        scenes.upload(c, spec)
        c.set_schedule(schedule)
        g = gbuffer(c, W, H)
        nhit = check_against_oracle(g, name)
        assert 100 < nhit <= W * H
        nmodel = check_primary_frame(c, spec, g, name)
        assert nmodel > 20
    if name == "DEGEN":  # both hit groups and the mirrored instance are on screen
        assert set(np.unique(g["object"][g["hits"][:, 3] == 1, 0])) >= {1, 2, 5}
        assert set(np.unique(g["object"][g["hits"][:, 3] == 1, 1])) == {rt.RT_HITGROUP_MODEL, rt.RT_HITGROUP_PLANE}


@pytest.mark.parametrize("seed", [5, 9, 24, 46])
def test_random_scenes(seed):
    """Mirrored, scaled and rotated instances of both hit groups, indexed and non-indexed meshes, 96 x 64."""
    name = f"RND{seed}"
    spec = spec_of(name, 96, 64)
    with rt.Context(0) as c:
        scenes.upload(c, spec)
        g = gbuffer(c, 96, 64)
        assert check_against_oracle(g, name, 96, 64) > 200
        check_primary_frame(c, spec, g, name)


def test_every_pixel_a_miss_and_one_pixel_frames():
    with rt.Context(0) as c:
        scenes.upload(c, spec_of("AWAY"))
        g = gbuffer(c, W, H)
        assert check_against_oracle(g, "AWAY") == 0
        for name in ("AWAY", "C2F"):  # 1 x 1: a miss, a hit
            c.set_camera(spec_of(name, 1, 1).camera_buffer())
            for schedule in (PACKET, LANE):
                c.set_schedule(schedule)
                nhit = check_against_oracle(gbuffer(c, 1, 1), name, 1, 1, f"{name} 1 x 1")
                assert nhit == (1 if name == "C2F" else 0)


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [PACKET, LANE], ids=["packet", "lane"])
def test_row_lists_and_single_planes(schedule):
    rows = np.array([20, 3, 3, 11, 0], np.uint32)
    with rt.Context(0) as c:
        scenes.upload(c, spec_of("DEGEN"))
        c.set_schedule(schedule)
        full = gbuffer(c, W, H)
        check_against_oracle(full, "DEGEN")
        part = gbuffer(c, W, H, rows)
        for name, words in PLANES:
            want = full[name].reshape(H, W, words)[rows].reshape(-1, words)
            assert_plane(part[name], want, f"rows {name}")
            alone = gbuffer(c, W, H, rows, planes=(name,))
            assert list(alone) == [name]
            assert_plane(alone[name], want, f"{name} alone")


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [PACKET, LANE], ids=["default", "lane"])
def test_deep_trees(schedule):
    """DEEP's per-lane stack bound is past the 32 LDS entries, so the per-lane kernel runs on the launch's HBM
    overflow stack; its packet-stack bound (TLAS siblings + BLAS levels) stays below 64, so the default schedule
    still walks it as packets (test_packet_stack_fallback has the scene that does fall back). Either way the planes
    are the oracle's and, as for a frame, nothing overflows."""
    spec = spec_of("DEEP")
    with rt.Context(0) as c:
        ids = scenes.upload(c, spec)
        assert c.tlas_info().max_stack + 1 + c.blas_info(ids[0]).max_stack > 32
        if schedule == LANE:
            c.set_schedule(LANE)
        c.set_stats(True)
        c.set_tile_balance(0)
        g = gbuffer(c, W, H)
        sg = c.stats()
        assert check_against_oracle(g, "DEEP") > 100
        c.stats_reset()
        check_primary_frame(c, spec, g, "DEEP")
        sf = c.stats()
    assert sg["stack_overflows"] == 0 and sf["stack_overflows"] == 0
    assert sg["primary_rays"] == W * H


def chain_scene():
    """A scene whose PACKET-stack bound reaches 64, so the default schedule falls back to the per-lane kernel: 96
    instances of one large triangle with their centres on deep_chain_mesh's Morton chain (three per chain point:
    the TLAS's worst-case stack is 64 entries) behind them one instance of deep_chain_mesh itself (18 BLAS levels)."""
    rng = np.random.default_rng(5)
    cents = [np.full(3, 0.5), np.full(3, 1023.5)]
    for j in range(9, -1, -1):
        for ax in range(3):
            c = np.full(3, 0.5)
            c[ax] = 2 ** j + 0.5
            cents.append(c)
    tri = np.zeros((3, 6), np.float32)
    tri[:, :3] = [(-30.0, -30.0, 0.0), (30.0, -30.0, 0.0), (0.0, 30.0, 0.0)]
    tri[:, 4] = 1.0
    inst = []
    for c in cents:
        for _ in range(3):
            p = c / 1024.0 * 40.0 + rng.normal(scale=0.05, size=3)
            inst.append((0, scenes.translation(*(float(v) for v in p)), len(inst), rt.RT_HITGROUP_PLANE))
    inst.append((1, scenes.translation(0.0, 0.0, -3.0), len(inst), rt.RT_HITGROUP_MODEL))
    return scenes.SceneSpec("CHAIN", [(tri, None), (scenes.deep_chain_mesh(), None)], inst, scenes.REFERENCE_LIGHTS[:1],
                            scenes.REFERENCE_MATERIAL, ((20.0, 22.0, 70.0), (20.0, 18.0, 0.0), (0.0, 1.0, 0.0)), W, H,
                            rt.RT_SHADE_PRIMARY)


def test_packet_stack_fallback():
    """CHAIN under the default schedule: the packet-stack bound (TLAS siblings + BLAS levels) is 64 or more, so the
    launch runs the per-lane kernel, as a frame of the scene does: the planes are the oracle's, and every traversal
    counter (per lane in that kernel, per wave in the packet kernel) equals the RT_SCHED_LANE launch's and the
    PRIMARY frame's."""
    spec = spec_of("CHAIN")
    traversal = ("aabb_tests", "tri_tests", "instance_entries", "node_fetches", "tri_fetches", "instance_fetches")
    with rt.Context(0) as c:
        ids = scenes.upload(c, spec)
        assert c.tlas_info().max_stack + c.blas_info(ids[1]).depth >= 64
        c.set_tile_balance(0)
        c.set_stats(True)
        got = {}
        for schedule in (PACKET, LANE):
            c.set_schedule(schedule)
            c.stats_reset()
            assert check_against_oracle(gbuffer(c, W, H), "CHAIN") > 100
            got[schedule] = c.stats()
        c.set_schedule(PACKET)
        c.stats_reset()
        out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        c.dispatch(W, H, out8, stream=torch.cuda.current_stream().cuda_stream)
        frame = c.stats()
    for k in traversal + ("primary_rays", "stack_overflows"):
        assert got[PACKET][k] == got[LANE][k] == frame[k], f"{k}: {got[PACKET][k]}, {got[LANE][k]}, frame {frame[k]}"
    assert got[PACKET]["stack_overflows"] == 0 and got[PACKET]["node_fetches"] > W * H


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [PACKET, LANE], ids=["packet", "lane"])
def test_counters_equal_a_primary_frame(schedule):
    spec = spec_of("REF")
    traversal = ("aabb_tests", "tri_tests", "instance_entries", "node_fetches", "tri_fetches", "instance_fetches")
    with rt.Context(0) as c:
        scenes.upload(c, spec)
        c.set_shading(spec.lights, spec.material, rt.RT_SHADE_PRIMARY, 1)
        c.set_schedule(schedule)
        c.set_tile_balance(0)
        c.set_stats(True)
        out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        c.dispatch(W, H, out8, stream=torch.cuda.current_stream().cuda_stream)
        frame = c.stats()
        c.stats_reset()
        gbuffer(c, W, H)
        g = c.stats()
        c.stats_reset()
        rows = np.array([20, 3, 3, 11, 0], np.uint32)
        gbuffer(c, W, H, rows)
        part = c.stats()
    for k in traversal:
        assert g[k] == frame[k] and g[k] > 0, f"{k}: G-buffer {g[k]}, PRIMARY frame {frame[k]}"
    assert g["primary_rays"] == g["pixels"] == W * H == frame["primary_rays"]
    assert g["shadow_rays"] == 0 and g["reflection_rays"] == 0 and g["dispatches"] == 1 and g["stack_overflows"] == 0
    assert part["primary_rays"] == part["pixels"] == rows.size * W and part["dispatches"] == 1


# 6 ------------------------------------------------------------------------------------------------
def test_watertight_mode():
    spec = spec_of("DEGEN")
    rays = pixel_rays(spec)
    n = rays.shape[0]
    with rt.Context(0) as c:
        scenes.upload(c, spec)
        c.set_triangle_test(rt.RT_TRIANGLE_TEST_WATERTIGHT)
        d_rays = torch.from_numpy(rays).cuda()
        hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        uv = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        c.trace_rays(d_rays, n, False, hits, uv, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want_hits, want_uv = hits.cpu().numpy().view(np.uint32), uv.cpu().numpy().view(np.uint32)
        for schedule in (PACKET, LANE):
            c.set_schedule(schedule)
            g = gbuffer(c, W, H)
            assert_plane(g["hits"], want_hits, "watertight hits")
            assert_plane(g["uv"], want_uv, "watertight uv")
            assert_plane(g["normal"], host_normals(spec, g["hits"], g["uv"]), "watertight normal")
            assert_plane(g["object"], objects_of(spec, g["hits"]), "watertight object")
        assert (want_uv != oracle_planes("DEGEN")[1]).any()  # the two tests differ in their last bits
        c.set_triangle_test(rt.RT_TRIANGLE_TEST_MOLLER_TRUMBORE)
        check_against_oracle(gbuffer(c, W, H), "DEGEN", what="back to Moller-Trumbore")


# 7 ------------------------------------------------------------------------------------------------
def test_refit_needs_a_tlas_build():
    spec = spec_of("C2F")
    with rt.Context(0) as c:
        ids = scenes.upload(c, spec)
        c.blas_refit(ids[0], spec.meshes[0][0])
        with pytest.raises(rt.RtError) as e:
            gbuffer(c, W, H)
        assert e.value.status == rt.RT_E_INVALID and "refit" in str(e.value)
        c.tlas_build([(ids[m], x, iid, hg) for (m, x, iid, hg) in spec.instances], update_only=True)
        check_against_oracle(gbuffer(c, W, H), "C2F", what="after the update")


def test_tlas_update_between_launches_on_two_streams():
    """A on stream 1, a TLAS update that moves the instances, B on stream 2, no host synchronisation in between:
    A sees the old transforms, B the new ones (the TLAS double buffer notes G-buffer launches as it notes frames)."""
    old = spec_of("C2F")
    new = scenes.SceneSpec(**{**old.__dict__})
    new.instances = [(0, scenes.translation(0.75, 0.5, -0.5), 0, rt.RT_HITGROUP_MODEL),
                     (1, scenes.translation(0.0, -0.25, 0.0), 1, rt.RT_HITGROUP_PLANE)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with rt.Context(0) as c:
        ids = scenes.upload(c, old)
        a, b = alloc(W, H), alloc(W, H)
        torch.cuda.synchronize()  # the fills are done; from here on no host wait until both launches are issued
        launch(c, W, H, a, stream=s1)
        c.tlas_build([(ids[m], x, iid, hg) for (m, x, iid, hg) in new.instances], update_only=True)
        launch(c, W, H, b, stream=s2)
        torch.cuda.synchronize()
        ga, gb = collect(a), collect(b)
        c.forget_stream(s1.cuda_stream)
        c.forget_stream(s2.cuda_stream)
    check_against_oracle(ga, "C2F", what="before the update")
    hits, uv, _ = oracle.Scene(new).trace_rays(pixel_rays(new))
    assert_plane(gb["hits"], hits, "after the update: hits")
    assert_plane(gb["uv"], uv.view(np.uint32), "after the update: uv")
    assert_plane(gb["normal"], host_normals(new, gb["hits"], gb["uv"]), "after the update: normal")
    assert_plane(gb["object"], objects_of(new, hits), "after the update: object")
    assert (ga["hits"] != gb["hits"]).any()


def test_no_shading_state_needed():
    spec = spec_of("REF")
    with rt.Context(0) as c:
        ids = [c.blas_build(v, i) for (v, i) in spec.meshes]
        c.tlas_build([(ids[m], x, iid, hg) for (m, x, iid, hg) in spec.instances])
        c.set_camera(spec.camera_buffer())
        check_against_oracle(gbuffer(c, W, H), "REF", what="no rt_set_shading")
        out8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        with pytest.raises(rt.RtError):  # a frame does need it
            c.dispatch(W, H, out8)


def test_error_cases_write_nothing():
    spec = spec_of("C2F")
    n = W * H
    bufs = {name: torch.full((n * words,), int(FILL.view(np.int32)), dtype=torch.int32, device="cuda")
            for name, words in PLANES}
    g = rt.rt_gbuffer(*[bufs[name].data_ptr() for name, _ in PLANES])
    rows5 = (ctypes.c_uint32 * 5)(20, 3, 3, 11, 0)
    bad_row = (ctypes.c_uint32 * 2)(0, H)

    def call(c, w=W, h=H, rows=None, nrows=H, out=g):
        return c._lib.rt_dispatch_gbuffer(c._h, w, h, rows, nrows, None if out is None else ctypes.byref(out), None)

    with rt.Context(0) as c:  # no TLAS, then no camera
        c.set_camera(spec.camera_buffer())
        assert call(c) == rt.RT_E_INVALID and b"TLAS" in c._lib.rt_last_error(c._h)
    with rt.Context(0) as c:
        scenes.upload(c, spec, camera=False)
        assert call(c) == rt.RT_E_INVALID and b"camera" in c._lib.rt_last_error(c._h)
        c.set_camera(spec.camera_buffer())
        assert call(c, out=None) == rt.RT_E_INVALID
        assert call(c, out=rt.rt_gbuffer()) == rt.RT_E_INVALID and b"null" in c._lib.rt_last_error(c._h)
        assert call(c, w=0) == rt.RT_E_INVALID and call(c, h=0) == rt.RT_E_INVALID
        assert call(c, rows=rows5, nrows=0) == rt.RT_E_INVALID
        assert call(c, rows=bad_row, nrows=2) == rt.RT_E_INVALID and b"row" in c._lib.rt_last_error(c._h)
        odd = rt.rt_gbuffer(bufs["hits"].data_ptr() + 4, None, None, None)
        assert call(c, out=odd) == rt.RT_E_INVALID and b"aligned" in c._lib.rt_last_error(c._h)
        with pytest.raises(ValueError):  # the Python layer checks the element counts
            c.dispatch_gbuffer(W, H, hits=bufs["uv"])
        with pytest.raises(ValueError):
            c.dispatch_gbuffer(W, H, uv=torch.zeros((n, 2), dtype=torch.float64, device="cuda"))
        torch.cuda.synchronize()
        for name, _ in PLANES:
            assert (bufs[name].cpu().numpy().view(np.uint32) == FILL).all(), f"{name} written by a refused call"
        assert call(c, rows=rows5, nrows=5) == rt.RT_OK  # and the same buffers are fine for a valid call
        torch.cuda.synchronize()


# the library variants (Makefile VARIANTS): every code-shape knob the G-buffer kernels compile under
@pytest.mark.parametrize("var", ["n1", "n1root", "rays2", "alt", "wavetimes", "ldstop", "popcullblas", "popcullstats"])
def test_variant_libraries(var):
    path = os.path.join(os.path.dirname(rt.LIB_PATH), "variants", var, "librtamd.so")
    assert os.path.exists(path), f"{path} missing: `make` builds the variants (no fallback)"
    with rt.Context(0, library=rt._load(path)) as c:
        scenes.upload(c, spec_of("DEGEN"))
        for stats in (False, True):  # the plain and the counting kernels
            c.set_stats(stats)
            for schedule in (PACKET, LANE):
                c.set_schedule(schedule)
                check_against_oracle(gbuffer(c, W, H), "DEGEN", what=f"{var} stats {stats} schedule {schedule}")
        assert c.stats()["stack_overflows"] == 0


# 8 ------------------------------------------------------------------------------------------------
def test_pick():
    spec = spec_of("DEGEN")
    with rt.Context(0) as c:
        scenes.upload(c, spec)
        g = gbuffer(c, W, H)
        hit = np.nonzero(g["hits"][:, 3] == 1)[0]
        miss = np.nonzero(g["hits"][:, 3] == 0)[0]
        assert hit.size and miss.size
        for p in (int(hit[hit.size // 2]), int(miss[0]), W * H - 1):
            got = c.pick(W, H, p % W, p // W)
            if g["hits"][p, 3] == 0:
                assert got is None
                continue
            f = lambda a: a.view(np.float32)  # noqa: E731
            assert got == {"t": float(f(g["hits"][p, 0:1])[0]), "instance_id": int(g["hits"][p, 1]),
                           "instance": int(g["object"][p, 0]), "hit_group": int(g["object"][p, 1]),
                           "primitive": int(g["hits"][p, 2]), "uv": tuple(float(v) for v in f(g["uv"][p])),
                           "normal": tuple(float(v) for v in f(g["normal"][p, :3]))}
        with pytest.raises(ValueError):
            c.pick(W, H, W, 0)
