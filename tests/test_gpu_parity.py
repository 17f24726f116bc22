"""GPU parity: the HIP path (through the C-ABI) against the CPU oracle on the same inputs.

Integer/index work (BVH nodes, leaf order, hit ids, RGBA8) must match bit for bit; the float32
frame too, because the kernel and the oracle evaluate the same expressions in the same order with
correctly rounded IEEE operations (-ffp-contract=off on both sides). The tolerance written into the
float checks below is 0 for that reason; BASELINE's north-star bound (L-inf < 1e-3) is far looser.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import realtimeraytracing_gradproject_amd as rt  # noqa: E402
from realtimeraytracing_gradproject_amd import scenes  # noqa: E402

import oracle  # noqa: E402

FLOAT_TOL = 0.0  # bit-identical float32 frame expected (north-star bound: 1e-3)


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def fresh_ctx():
    return rt.Context(0)


def gpu_render(c, spec, rows=None, schedule=rt.RT_SCHED_PACKET):
    nrows = spec.height if rows is None else len(rows)
    out8 = torch.empty((nrows, spec.width, 4), dtype=torch.uint8, device="cuda")
    out32 = torch.empty((nrows, spec.width, 4), dtype=torch.float32, device="cuda")
    c.set_schedule(schedule)
    c.dispatch(spec.width, spec.height, out8, out32, rows=rows, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out8.cpu().numpy(), out32.cpu().numpy()


def load_both(spec):
    c = fresh_ctx()
    scenes.upload(c, spec)
    o = oracle.Scene(spec)
    return c, o


def assert_images_equal(g8, g32, o8, o32, what):
    d = np.abs(g32.astype(np.float64) - o32.astype(np.float64))
    bad = np.argwhere(d > FLOAT_TOL)
    assert d.max() <= FLOAT_TOL, f"{what}: float L-inf {d.max()} at {bad[:5].tolist()} ({len(bad)} values)"
    n8 = int((g8 != o8).sum())
    assert n8 == 0, f"{what}: {n8} RGBA8 channels differ"


# ------------------------------------------------------------------------------------------
# acceleration structures
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["teapot", "rabbit"])
def test_blas_bitwise_equal_to_oracle(model):
    v, i = scenes.load_model(model)
    c = fresh_ctx()
    b = c.blas_build(v, i)
    gn, gt = c.blas_export(b)
    o = oracle.Scene()
    ob = o.add_blas(v, i)
    on, ot = o.export_blas(ob)
    assert np.array_equal(gn, on), f"{model}: {int((gn != on).any(axis=1).sum())} nodes differ"
    assert np.array_equal(gt, ot)
    info = c.blas_info(b)
    prims, nn, depth, mstack = o.blas_info(ob)
    assert (info.prim_count, info.node_count, info.depth, info.max_stack) == (prims, nn, depth, mstack)
    # every primitive exactly once in leaf order
    assert np.array_equal(np.sort(gt[:, 3]), np.arange(prims, dtype=np.uint32))
    c.close()


# 1: the one-node kernel (k_build_one); 2 .. 512: the one-launch LDS build (k_build_tiny);
# 513 .. 8192: the four-launch build (k_mid_*, block boundaries at 1024-leaf multiples); 8193 and
# 20000: the multi-kernel build
@pytest.mark.parametrize("ntri", [1, 2, 3, 7, 63, 64, 65, 512, 513, 1000, 1023, 1024, 1025, 2049, 5000, 8191, 8192,
                                  8193, 20000])
def test_blas_edge_sizes(ntri):
    rng = np.random.default_rng(1234 + ntri)
    v = np.zeros((ntri * 3, 6), np.float32)
    v[:, :3] = rng.uniform(-5, 5, size=(ntri * 3, 3)).astype(np.float32)
    v[:, 4] = 1.0
    c = fresh_ctx()
    b = c.blas_build(v)  # non-indexed
    gn, gt = c.blas_export(b)
    o = oracle.Scene()
    ob = o.add_blas(v)
    on, ot = o.export_blas(ob)
    assert np.array_equal(gn, on)
    assert np.array_equal(gt, ot)
    c.close()


@pytest.mark.parametrize("ntri", [1, 2, 100, 1025, 3000, 8192, 8193])
def test_build_schedules_bitwise_equal(ntri, monkeypatch):
    # every schedule that can hold n (RT_BUILD_PATH: one-launch LDS build for 2 <= n <= 512, four launches
    # for 2 <= n <= 8192, multi-kernel; a schedule that cannot hold n falls back to the default) builds the
    # oracle's tree, BLAS and TLAS alike. n = 1: the one-node kernel (the fallback of tiny and mid) and the
    # forced multi-kernel build, for a 1-triangle BLAS and a 1-instance TLAS; 8193: every value ends in multi
    rng = np.random.default_rng(77 + ntri)
    v = np.zeros((ntri * 3, 6), np.float32)
    c0 = rng.uniform(-5, 5, size=(ntri, 1, 3))
    v[:, :3] = (c0 + rng.uniform(-0.3, 0.3, size=(ntri, 3, 3))).reshape(-1, 3).astype(np.float32)
    o = oracle.Scene()
    ob = o.add_blas(v)
    on, ot = o.export_blas(ob)
    ninst = min(ntri, 600)
    inst = [(0, scenes._rot_scale((0.0, 1.0, 0.0), float(k % 7) * 10.0, (1.0, 1.0, 1.0),
                                  tuple(rng.integers(-30, 30, size=3).astype(np.float64))), k, 0)
            for k in range(ninst)]
    o.set_instances([(ob, x, iid, hg) for (_, x, iid, hg) in inst])
    otl = o.export_tlas()
    for path in ("tiny", "mid", "multi"):
        monkeypatch.setenv("RT_BUILD_PATH", path)
        c = fresh_ctx()
        b = c.blas_build(v)
        gn, gt = c.blas_export(b)
        assert np.array_equal(gn, on) and np.array_equal(gt, ot), f"{path}: BLAS differs"
        c.tlas_build([(b, x, iid, hg) for (_, x, iid, hg) in inst])
        assert np.array_equal(c.tlas_export(), otl), f"{path}: TLAS differs"
        c.close()


def test_one_triangle_tree_traced_and_refitted():
    # the consumers of the one-node tree: the walk (a 1-triangle BLAS under a 1-instance TLAS), the refit's parent
    # table and its one-workgroup climb
    v = np.zeros((3, 6), np.float32)
    v[:, :3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    v[:, 4] = 1.0
    x = scenes.translation(1.0, 2.0, 3.0)
    rays = np.zeros((8, 8), np.float32)
    # four rays down -z through the triangle, three beside it, one through it but pointing away
    rays[:, :2] = [[0.2, 0.2], [0.1, 0.6], [0.6, 0.1], [0.3, 0.3], [0.8, 0.8], [-0.5, 0.2], [2.0, 2.0], [0.2, 0.2]]
    rays[:, :3] += [1.0, 2.0, 8.0]
    rays[:, 6] = -1.0
    rays[7, 6] = 1.0
    rays[:, 7] = 100000.0
    o = oracle.Scene()
    ob = o.add_blas(v)
    o.set_instances([(ob, x, 0, 0)])
    oh, ouv, _ = o.trace_rays(rays, any_hit=False)
    assert oh[:, 3].tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
    c = fresh_ctx()
    b = c.blas_build(v)
    c.tlas_build([(b, x, 0, 0)])
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.zeros((8, 4), dtype=torch.int32, device="cuda")
    d_uv = torch.zeros((8, 2), dtype=torch.float32, device="cuda")
    c.trace_rays(d_rays, 8, False, d_hits, d_uv, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), oh)
    assert np.array_equal(d_uv.cpu().numpy(), ouv)
    n0, t0 = c.blas_export(b)
    c.blas_refit(b, v)  # the build's own vertices: the build's bytes
    n1, t1 = c.blas_export(b)
    assert n1.tobytes() == n0.tobytes() and t1.tobytes() == t0.tobytes()
    moved = v.copy()
    moved[:, :3] = [[0.5, -1.0, 2.0], [3.0, 0.25, -0.0], [-2.0, 4.0, 1.5]]
    c.blas_refit(b, moved)
    n2, t2 = c.blas_export(b)
    c2 = fresh_ctx()
    fn, ft = c2.blas_export(c2.blas_build(moved))
    assert n2.tobytes() == fn.tobytes() and t2.tobytes() == ft.tobytes()
    c2.close()
    c.close()


@pytest.mark.parametrize("mesh", ["soup", "point"])
def test_blas_degenerate_geometry(mesh):
    # zero-area, point, duplicate, sliver and flat triangles; a BLAS with zero extent on every axis
    v = scenes.degenerate_soup() if mesh == "soup" else scenes.point_cloud_mesh()
    c = fresh_ctx()
    gn, gt = c.blas_export(c.blas_build(v))
    o = oracle.Scene()
    on, ot = o.export_blas(o.add_blas(v))
    assert np.array_equal(gn, on) and np.array_equal(gt, ot)
    c.close()


@pytest.mark.parametrize("count", [300, 512, 513, 1025, 3000, 8192, 9000])
def test_blas_duplicate_centroids(count):
    # many triangles with identical Morton codes: Karras tie-break on leaf position; the sort must
    # stay stable across waves and across every build schedule (tiny <= 512 < mid <= 8192 < multi)
    v = np.zeros((count * 3, 6), np.float32)
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    for k in range(count):
        v[k * 3:(k + 1) * 3, :3] = base
    c = fresh_ctx()
    b = c.blas_build(v)
    gn, gt = c.blas_export(b)
    o = oracle.Scene()
    ob = o.add_blas(v)
    on, ot = o.export_blas(ob)
    assert np.array_equal(gn, on) and np.array_equal(gt, ot)
    c.close()


@pytest.mark.parametrize("name", ["REF", "C4", "DEGEN"])
def test_tlas_bitwise_equal_to_oracle(name):
    spec = scenes.config(name)
    c, o = load_both(spec)
    assert np.array_equal(c.tlas_export(), o.export_tlas())
    info = c.tlas_info()
    assert (info.prim_count, info.node_count, info.depth, info.max_stack) == tuple(o.tlas_info())
    c.close()


@pytest.mark.parametrize("ninst", [1, 3, 1024, 8192, 9000])
def test_tlas_instance_counts(ninst):
    # TLAS over ninst instances of one small mesh at seeded translations / rotations (coincident
    # boxes included): tiny (<= 512), four-launch (<= 8192) and multi-kernel (9000) builds against
    # the oracle
    rng = np.random.default_rng(ninst)
    v = np.array([[0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, 0], [0, 1, 0, 0, 1, 0],
                  [0, 0, 1, 0, 1, 0], [1, 1, 1, 0, 1, 0], [0, 1, 1, 0, 1, 0]], np.float32)
    inst = []
    for k in range(ninst):
        t = rng.integers(-40, 40, size=3).astype(np.float64) * 0.5
        x = scenes._rot_scale((0.0, 1.0, 0.0), float(k % 90) if k % 3 == 1 else 0.0, (1.0, 1.0, 1.0), t)
        inst.append((0, x, k, 0))
    c = fresh_ctx()
    b = c.blas_build(v)
    c.tlas_build([(b, x, iid, hg) for (_, x, iid, hg) in inst])
    o = oracle.Scene()
    ob = o.add_blas(v)
    o.set_instances([(ob, x, iid, hg) for (_, x, iid, hg) in inst])
    assert np.array_equal(c.tlas_export(), o.export_tlas())
    info = c.tlas_info()
    assert (info.prim_count, info.node_count, info.depth, info.max_stack) == tuple(o.tlas_info())
    c.close()


# ------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------

SMALL = {"REF": (160, 90), "C1": (128, 128), "C2": (192, 108), "C3": (192, 108), "C4": (192, 108),
         "C5": (96, 54), "REFL": (160, 90), "REFLO": (160, 90), "DEGEN": (320, 180), "DEEP": (96, 64)}


SCHEDULES = {"packet": rt.RT_SCHED_PACKET, "lane": rt.RT_SCHED_LANE}


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("name", list(SMALL))
def test_frame_parity_small(name, sched):
    spec = scenes.config(name).with_size(*SMALL[name])
    c, o = load_both(spec)
    g8, g32 = gpu_render(c, spec, schedule=SCHEDULES[sched])
    o8, o32, _ = o.render_spec(spec, nthreads=8)
    assert_images_equal(g8, g32, o8, o32, f"{name}/{sched}")
    c.close()


RAGGED = [(1, 1), (1, 19), (23, 1), (7, 3), (65, 9), (9, 65), (129, 17)]


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("spp", [1, 4, 9])
def test_ragged_frame_sizes(sched, spp):
    """Frames whose sides are not multiples of the 8 x 8 (or 4 x 4 pixels x 4 samples) wave tile: single pixels,
    single rows and columns, odd rectangles -- the lanes outside the image must neither write nor change the
    packet walk of the lanes inside. Every kernel variant: one sample, the sample-lane kernel (4 spp) and the
    sample loop (9 spp), both schedules; C4 (two lights, 65 instances) under the reference camera's grid view."""
    base = scenes.config("C4")
    c = fresh_ctx()
    scenes.upload(c, base.with_size(64, 36))
    o = oracle.Scene(base)
    for (w, h) in RAGGED:
        spec = base.with_size(w, h)
        spec.spp = spp
        c.set_camera(spec.camera_buffer())
        c.set_shading(spec.lights, spec.material, spec.mode, spec.spp)
        g8, g32 = gpu_render(c, spec, schedule=SCHEDULES[sched])
        o8, o32, _ = o.render_spec(spec, nthreads=4)
        assert_images_equal(g8, g32, o8, o32, f"C4 {w}x{h} spp {spp} {sched}")
    c.close()


def sweep_cameras(n, seed=0x5EED):
    """a seeded camera sweep. Eyes on spheres of radius 0.5..40 around points near the
    scene (some inside a model, some grazing the plane), looking at random targets; random up
    vectors (never parallel to the view direction)."""
    rng = np.random.default_rng(seed)
    cams = []
    while len(cams) < n:
        c = rng.uniform([-6, -0.5, -6], [6, 3, 6])
        d = rng.normal(size=3)
        eye = c + d / np.linalg.norm(d) * rng.choice([0.5, 2.0, 8.0, 20.0, 40.0])
        up = rng.normal(size=3)
        f = c - eye
        if abs(np.dot(up, f)) / (np.linalg.norm(up) * np.linalg.norm(f)) > 0.95:
            continue
        cams.append((tuple(float(v) for v in eye), tuple(float(v) for v in c), tuple(float(v) for v in up)))
    return cams


@pytest.mark.parametrize("name", ["REF", "C2", "C4", "REFL", "DEGEN"])
def test_camera_sweep_matches_oracle(name):
    """GPU frame == oracle frame (RGBA8 and float32, bit for bit) and packet counters equal, for 8
    seeded cameras per scene, one of them with 4 spp and one as a non-square odd-sized target."""
    base = scenes.config(name)
    c = fresh_ctx()
    scenes.upload(c, base.with_size(64, 36))
    o = oracle.Scene(base)
    for k, cam in enumerate(sweep_cameras(8, 0x5EED + k_offset(name))):
        spec = base.with_size(*((61, 37) if k == 5 else (64, 36)))
        spec.camera = cam
        spec.spp = 4 if k == 3 else 1
        c.set_camera(spec.camera_buffer())
        c.set_shading(spec.lights, spec.material, spec.mode, spec.spp)
        c.set_stats(True)
        c.stats_reset()
        g8, g32 = gpu_render(c, spec)
        gst = c.stats()
        c.set_stats(False)
        o8, o32, ost = o.render_spec(spec, nthreads=8)
        assert_images_equal(g8, g32, o8, o32, f"{name}/camera {k}")
        assert gst["aabb_tests"] == int(ost[2]) and gst["tri_tests"] == int(ost[3]), f"{name}/camera {k}"
    c.close()


def k_offset(name):
    return sum(ord(ch) for ch in name)


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("name", ["REF", "C2", "C2F", "C4", "C5", "REFL", "REFLO", "DEGEN"])
def test_counters_match_oracle(name, sched):
    """Traversal counters equal the oracle's emulation of the same schedule: same visit order."""
    spec = scenes.config(name).with_size(*SMALL.get(name, (192, 108)))
    c, o = load_both(spec)
    c.set_stats(True)
    c.stats_reset()
    gpu_render(c, spec, schedule=SCHEDULES[sched])
    s = c.stats()
    _, _, ost = o.render_spec(spec, nthreads=8, schedule=SCHEDULES[sched])
    keys = ["primary_rays", "shadow_rays", "aabb_tests", "tri_tests", "instance_entries", "stack_overflows"]
    assert [s[k] for k in keys] == [int(x) for x in ost[:6]]
    assert s["reflection_rays"] == int(ost[8])
    # record fetches (the roofline's byte counts): per wave in packets, per lane per ray
    assert [s[k] for k in ["node_fetches", "tri_fetches", "instance_fetches"]] == [int(x) for x in ost[9:12]]
    assert s["stack_overflows"] == 0
    c.close()


def test_packet_counters_on_row_subset():
    """Packet tiles follow the row list (8 list entries per tile row), as the oracle emulates."""
    spec = scenes.config("C2").with_size(160, 96)
    c, o = load_both(spec)
    rows = np.array([1, 2, 3, 7, 11, 12, 40, 41, 42, 60, 61, 90, 95], np.uint32)
    c.set_stats(True)
    c.stats_reset()
    g8, g32 = gpu_render(c, spec, rows=rows)
    s = c.stats()
    o8, o32, ost = o.render_spec(spec, rows=rows, nthreads=4)
    assert_images_equal(g8, g32, o8, o32, "row subset")
    assert [s[k] for k in ["primary_rays", "shadow_rays", "aabb_tests", "tri_tests"]] == [int(x) for x in ost[:4]]
    c.close()


def test_rows_subset_matches_full_frame():
    spec = scenes.config("C2").with_size(160, 96)
    c, o = load_both(spec)
    f8, f32 = gpu_render(c, spec)
    rows = np.array([0, 5, 17, 18, 50, 95], np.uint32)
    r8, r32 = gpu_render(c, spec, rows=rows)
    assert np.array_equal(r8, f8[rows]) and np.array_equal(r32, f32[rows])
    c.close()


@pytest.mark.parametrize("name,size", [("C2", (150, 93)), ("C4", (200, 101)), ("REF", (96, 54)), ("REFL", (64, 37)),
                                       ("C5", (48, 27)), ("C2", (7, 3))])
def test_tile_rows_4_matches_oracle(name, size):
    """rt_set_tile_rows(4) (8 x 4 pixel tiles per wave, half the lanes idle) renders the oracle's image, whole
    frames with ragged heights and a strip row list; multi-sample frames (C5) ignore the setting."""
    spec = scenes.config(name).with_size(*size)
    c, o = load_both(spec)
    c.set_tile_rows(4)
    g8, g32 = gpu_render(c, spec)
    o8, o32, _ = o.render_spec(spec, nthreads=8)
    assert_images_equal(g8, g32, o8, o32, f"{name} tile rows 4")
    rows = rt.strip_rows(spec.height, 3, 1) if spec.height > 8 else np.array([2, 0], np.uint32)
    r8, r32 = gpu_render(c, spec, rows=rows)
    assert np.array_equal(r8, o8[rows]) and np.array_equal(r32, o32[rows])
    c.set_tile_rows(8)
    f8, _ = gpu_render(c, spec)
    assert np.array_equal(f8, g8)
    with pytest.raises(rt.RtError):
        c.set_tile_rows(2)
    c.close()


@pytest.mark.parametrize("name", ["C2", "C2F", "C3", "C4", "C5", "REF", "REFL"])
def test_full_size_whole_frame(name):
    """Full BASELINE sizes (C2-C4 1920x1080, C5 3840x2160 at 4 spp, the reference scene 1280x720, with and
    without reflections): the WHOLE GPU frame against the whole oracle frame, float32 and RGBA8, bit for bit
    (every pixel, no row sample). The oracle renders with the per-ray schedule (the image does
    not depend on the schedule) on the box's 16-CPU share."""
    spec = scenes.config(name)
    c, o = load_both(spec)
    g8, g32 = gpu_render(c, spec)
    o8, o32, _ = o.render_spec(spec, nthreads=16, schedule=1)
    assert_images_equal(g8, g32, o8, o32, f"{name} {spec.width}x{spec.height} whole frame")
    # size-independent property: alpha channel is opaque everywhere
    assert (g8[..., 3] == 255).all()
    c.close()


def test_strip_partition_and_assemble():
    """Multi-GPU frame assembly on one device: render per-rank strips, gather, un-interleave."""
    spec = scenes.config("C2").with_size(200, 123)
    c, o = load_both(spec)
    full8, _ = gpu_render(c, spec)
    nranks, strip = 3, 8
    per = [rt.strip_rows(spec.height, nranks, r, strip) for r in range(nranks)]
    rows_per_rank = rt.strip_rows_per_rank(spec.height, nranks, strip)
    gathered = torch.zeros((nranks, rows_per_rank, spec.width, 4), dtype=torch.uint8, device="cuda")
    for r, rows in enumerate(per):
        part8, _ = gpu_render(c, spec, rows=rows)
        gathered[r, :len(rows)] = torch.from_numpy(part8).cuda()
    out = torch.empty((spec.height, spec.width, 4), dtype=torch.uint8, device="cuda")
    c.assemble_strips(spec.width, spec.height, nranks, strip, gathered, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), full8)
    c.close()


# ------------------------------------------------------------------------------------------
# TraceRay semantics: BVH closest hit == brute force over every triangle
# ------------------------------------------------------------------------------------------

def random_rays(n, seed, center=(0.0, 1.0, 0.0), radius=12.0):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * radius + np.asarray(center)
    tgt = rng.uniform(-6, 6, size=(n, 3)) + np.asarray(center)
    d = tgt - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = o
    rays[:, 3] = 0.0
    rays[:, 4:7] = d
    rays[:, 7] = 100000.0
    return rays


@pytest.mark.parametrize("any_hit,cull", [(False, False), (True, False), (False, True)])
def test_trace_rays_equals_bruteforce(any_hit, cull):
    spec = scenes.config("REF")
    c, o = load_both(spec)
    n = 100000
    rays = random_rays(n, 0x5EED)
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d_uv = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    c.trace_rays(d_rays, n, any_hit, d_hits, d_uv, cull_back=cull, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = d_hits.cpu().numpy().view(np.uint32)
    guv = d_uv.cpu().numpy()
    ob, ouv, _ = o.trace_rays(rays, any_hit=any_hit, brute_force=False, cull_back=cull)
    assert np.array_equal(g, ob), "GPU BVH traversal differs from oracle BVH traversal"
    assert np.array_equal(guv, ouv)
    if not any_hit:
        sub = slice(0, 20000)  # brute force is O(rays x triangles) on the CPU
        bb, buv, _ = o.trace_rays(rays[sub], any_hit=False, brute_force=True, cull_back=cull)
        assert np.array_equal(g[sub], bb), "BVH closest hit differs from brute force"
        assert np.array_equal(guv[sub], buv)
    else:
        bb, _, _ = o.trace_rays(rays[:20000], any_hit=True, brute_force=True)
        assert np.array_equal(g[:20000, 3], bb[:, 3]), "occlusion flag differs from brute force"
    assert g[:, 3].sum() > n // 10  # the sample actually hits geometry
    c.close()


@pytest.mark.parametrize("any_hit", [False, True])
def test_large_soup_multi_kernel_build_and_trace(any_hit):
    """60 K-triangle soup (the multi-kernel LBVH build, deep trees) under a rotated + scaled instance and
    a translated copy: tree bitwise equal to the oracle's, 50 K rays' hits equal the oracle's BVH
    walk (itself == brute force on smaller scenes) and, for 2 K of them, the oracle's brute force."""
    rng = np.random.default_rng(60000)
    ntri = 60000
    c0 = rng.uniform(-4, 4, size=(ntri, 1, 3))
    v = np.zeros((ntri * 3, 6), np.float32)
    v[:, :3] = (c0 + rng.normal(scale=0.08, size=(ntri, 3, 3))).reshape(-1, 3).astype(np.float32)
    v[:, 4] = 1.0
    inst = [(0, scenes._rot_scale((1.0, 2.0, 0.5), 33.0, (1.0, 0.7, 1.3), (0.0, 0.5, 0.0)), 0, 0),
            (0, scenes._rot_scale((0.0, 1.0, 0.0), 0.0, (1.0, 1.0, 1.0), (9.0, 0.0, -3.0)), 1, 0)]
    c = fresh_ctx()
    b = c.blas_build(v)
    c.tlas_build([(b, x, iid, hg) for (_, x, iid, hg) in inst])
    o = oracle.Scene()
    ob = o.add_blas(v)
    o.set_instances([(ob, x, iid, hg) for (_, x, iid, hg) in inst])
    gn, gt = c.blas_export(b)
    on, ot = o.export_blas(ob)
    assert np.array_equal(gn, on) and np.array_equal(gt, ot)
    n = 50000
    rays = random_rays(n, 0x5EED + 7)
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d_uv = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    c.trace_rays(d_rays, n, any_hit, d_hits, d_uv, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = d_hits.cpu().numpy().view(np.uint32)
    oh, ouv, _ = o.trace_rays(rays, any_hit=any_hit)
    assert np.array_equal(g, oh)
    if not any_hit:
        assert np.array_equal(d_uv.cpu().numpy(), ouv)
    bb, _, _ = o.trace_rays(rays[:2000], any_hit=any_hit, brute_force=True)
    assert np.array_equal(g[:2000, 3], bb[:, 3])
    if not any_hit:
        assert np.array_equal(g[:2000], bb)
    assert g[:, 3].sum() > n // 20
    c.close()


@pytest.mark.parametrize("any_hit,cull", [(False, None), (True, None), (False, "back"), (False, "front")])
def test_trace_rays_degenerate_and_transformed(any_hit, cull):
    """DEGEN: degenerate triangles under rotated, scaled and mirrored instances (the mirrored one
    swaps the culled face), plus a zero-extent BLAS: GPU == oracle BVH == brute force."""
    spec = scenes.config("DEGEN")
    c, o = load_both(spec)
    n = 60000
    rays = random_rays(n, 0xDE6E, center=(0.0, 1.0, 1.0), radius=14.0)
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d_uv = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    c.trace_rays(d_rays, n, any_hit, d_hits, d_uv, cull_back=cull == "back", cull_front=cull == "front", stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = d_hits.cpu().numpy().view(np.uint32)
    guv = d_uv.cpu().numpy()
    kw = dict(any_hit=any_hit, cull_back=cull == "back", cull_front=cull == "front")
    ob, ouv, _ = o.trace_rays(rays, **kw)
    assert np.array_equal(g, ob) and np.array_equal(guv, ouv)
    sub = slice(0, 8000)
    bb, buv, _ = o.trace_rays(rays[sub], brute_force=True, **kw)
    if any_hit:
        assert np.array_equal(g[sub, 3], bb[:, 3])
    else:
        assert np.array_equal(g[sub], bb) and np.array_equal(guv[sub], buv)
    assert len(np.unique(g[g[:, 3] == 1, 1])) >= 4  # rays reach most instances
    c.close()


# ------------------------------------------------------------------------------------------
# dynamic scenes and error behaviour
# ------------------------------------------------------------------------------------------

def test_blas_rebuild_and_tlas_update():
    spec = scenes.config("REF").with_size(128, 72)
    c, o = load_both(spec)  # BLAS ids on the device == mesh indices of the spec (0 model, 1 plane)
    rv, ri = scenes.load_model("rabbit")
    c.blas_rebuild(0, rv, ri)  # model hot-reload (D3D12HelloTriangle.cpp:1482-1596)
    c.tlas_build(spec.instances)
    spec2 = scenes.SceneSpec(**{**spec.__dict__})
    spec2.meshes = [(rv, ri), spec.meshes[1]]
    g8, g32 = gpu_render(c, spec2)
    o8, o32, _ = oracle.Scene(spec2).render_spec(spec2, nthreads=4)
    assert_images_equal(g8, g32, o8, o32, "after rebuild")
    # update_only: move instance 0, same BLAS ids (TopLevelASGenerator.cpp:202-222)
    inst = list(spec.instances)
    inst[0] = (0, scenes.translation(0.5, 0.25, -0.5), 0, rt.RT_HITGROUP_MODEL)
    c.tlas_build(inst, update_only=True)
    spec3 = scenes.SceneSpec(**{**spec2.__dict__})
    spec3.instances = inst
    g8, g32 = gpu_render(c, spec3)
    o8, o32, _ = oracle.Scene(spec3).render_spec(spec3, nthreads=4)
    assert_images_equal(g8, g32, o8, o32, "after TLAS update")
    with pytest.raises(rt.RtError):
        c.tlas_build(inst[:3], update_only=True)  # count change is not an update
    c.close()


def test_tlas_update_waits_for_frame_in_flight():
    """rt_tlas_build(update_only) overwrites the instance records and scene pools in
    place. A frame dispatched on a caller (torch) stream just before must still render the OLD
    scene: the build waits for in-flight work on every stream (quiesce), as the reference waits on
    its fence before rebuilding (D3D12HelloTriangle.cpp:1482-1568)."""
    spec = scenes.config("C4")  # 1080p, 65 instances: ~0.4 ms in flight
    c = fresh_ctx()
    scenes.upload(c, spec)
    ref8, _ = gpu_render(c, spec)
    moved = [(m, scenes.translation(float(x[3]) + 0.7, float(x[7]), float(x[11]) - 0.4) if hg == rt.RT_HITGROUP_MODEL
              else x, iid, hg) for (m, x, iid, hg) in spec.instances]
    s = torch.cuda.Stream()
    outs = []
    for _ in range(3):
        out = torch.empty((spec.height, spec.width, 4), dtype=torch.uint8, device="cuda")
        c.dispatch(spec.width, spec.height, out, None, stream=s.cuda_stream)
        outs.append(out)
    c.tlas_build(moved, update_only=True)  # no synchronisation by the caller in between
    after = torch.empty((spec.height, spec.width, 4), dtype=torch.uint8, device="cuda")
    c.dispatch(spec.width, spec.height, after, None, stream=s.cuda_stream)
    torch.cuda.synchronize()
    for k, out in enumerate(outs):
        assert np.array_equal(out.cpu().numpy(), ref8), f"frame {k} in flight saw the update"
    spec2 = scenes.SceneSpec(**{**spec.__dict__})
    spec2.instances = moved
    c2 = fresh_ctx()
    scenes.upload(c2, spec2)
    want8, _ = gpu_render(c2, spec2)
    assert np.array_equal(after.cpu().numpy(), want8)
    assert not np.array_equal(want8, ref8)
    c.close()
    c2.close()


def test_concurrent_deep_frames_on_streams():
    """VERDICT r2 #1 / ADVICE r2 (medium): launches in flight on different streams must not share device
    scratch. DEEP's per-lane stack bound exceeds the 32 LDS entries (the oracle's own walk reaches past
    them), so RT_SCHED_LANE frames use the HBM overflow stack. Three streams render three different cameras,
    each twice (full frame, then a strip row list of its own), and a fourth stream runs an rt_trace_rays
    batch, all enqueued with no synchronisation in between (the reference records and executes command lists
    asynchronously, D3D12HelloTriangle.cpp:436-456). Every frame and every hit equals the oracle's."""
    spec = scenes.config("DEEP").with_size(480, 320)
    c, o = load_both(spec)
    info = c.blas_info(0)
    assert c.tlas_info().max_stack + 1 + info.max_stack > 32  # the overflow stack is in use
    oracle.max_stack_reached()
    o.render_spec(spec.with_size(96, 64), nthreads=1, schedule=1)
    assert oracle.max_stack_reached() > 32  # ... and rays really go that deep
    c.set_schedule(rt.RT_SCHED_LANE)
    up = (0.0, 1.0, 0.0)
    cams = [spec.camera, ((26.0, 18.0, 64.0), (17.0, 19.0, 0.0), up), ((12.0, 26.0, 75.0), (23.0, 15.0, 3.0), up)]
    specs = []
    for cam in cams:
        sp = scenes.SceneSpec(**{**spec.__dict__})
        sp.camera = cam
        specs.append(sp)
    streams = [torch.cuda.Stream() for _ in range(4)]
    n = 40000
    rays = random_rays(n, 0xD33, center=(20.0, 18.0, 10.0), radius=60.0)
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    frames, parts = [], []
    for rnd in range(2):
        for k, sp in enumerate(specs):
            c.set_camera(sp.camera_buffer())
            f8 = torch.empty((sp.height, sp.width, 4), dtype=torch.uint8, device="cuda")
            f32 = torch.empty((sp.height, sp.width, 4), dtype=torch.float32, device="cuda")
            c.dispatch(sp.width, sp.height, f8, f32, stream=streams[k].cuda_stream)
            frames.append((k, f8, f32))
            if rnd == 0:
                c.trace_rays(d_rays, n, rnd == 1, d_hits, stream=streams[3].cuda_stream)
            rows = rt.strip_rows(sp.height, 3, k)
            p8 = torch.empty((len(rows), sp.width, 4), dtype=torch.uint8, device="cuda")
            c.dispatch(sp.width, sp.height, p8, None, rows=rows, stream=streams[k].cuda_stream)
            parts.append((k, rows, p8))
    torch.cuda.synchronize()
    want = [o.render_spec(sp, nthreads=8) for sp in specs]
    for k, f8, f32 in frames:
        assert_images_equal(f8.cpu().numpy(), f32.cpu().numpy(), want[k][0], want[k][1], f"DEEP camera {k}")
    for k, rows, p8 in parts:
        assert np.array_equal(p8.cpu().numpy(), want[k][0][rows]), f"DEEP camera {k} strip rows"
    oh, _, _ = o.trace_rays(rays, any_hit=False)
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), oh)
    assert len({int(np.abs(w[1]).sum()) for w in want}) == 3  # three different images
    c.close()


def test_raster_draws_on_two_streams():
    """back-to-back draws on different streams share the context's raster scratch; the second
    draw is ordered after the first on the device, so both images equal the oracle's."""
    spec = scenes.config("REF").with_size(320, 180)
    c, o = load_both(spec)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a8 = torch.empty((spec.height, spec.width, 4), dtype=torch.uint8, device="cuda")
    b8 = torch.empty((spec.height, spec.width, 4), dtype=torch.uint8, device="cuda")
    spec_b = scenes.SceneSpec(**{**spec.__dict__})
    spec_b.camera = ((9.0, 6.0, 11.0), (-1.5, 0.5, 0.0), (0.0, 1.0, 0.0))
    cb_a, cb_b = spec.camera_buffer(), spec_b.camera_buffer()
    c.raster_draw([0, 1], spec.width, spec.height, a8, stream=s1.cuda_stream)
    torch.cuda.synchronize()
    for _ in range(3):  # the same draw list (no re-upload), two cameras, two streams, no host sync
        c.set_camera(cb_a)
        c.raster_draw([0, 1], spec.width, spec.height, a8, stream=s1.cuda_stream)
        c.set_camera(cb_b)
        c.raster_draw([0, 1], spec.width, spec.height, b8, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    wa, _, _ = oracle.raster([spec.meshes[0], spec.meshes[1]], cb_a, spec.width, spec.height)
    wb, _, _ = oracle.raster([spec.meshes[0], spec.meshes[1]], cb_b, spec.width, spec.height)
    assert not np.array_equal(wa, wb)
    assert np.array_equal(a8.cpu().numpy(), wa)
    assert np.array_equal(b8.cpu().numpy(), wb)
    c.close()


def test_per_frame_tlas_update_with_frames_in_flight():
    """a per-frame TLAS update (OnUpdate -> TopLevelASGenerator update, D3D12HelloTriangle.cpp:421-433,
    TopLevelASGenerator.cpp:202-222) with three frames in flight: C5's 257 instances move every frame, each frame is
    dispatched on the next of three streams right after its update, with no host synchronisation in between. The
    double-buffered TLAS keeps every frame on its own instance set: each equals the oracle's render of that set."""
    spec = scenes.config("C5").with_size(192, 108)
    c = fresh_ctx()
    scenes.upload(c, spec)
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs, specs, walls = [], [], []
    for k in range(7):
        inst = []
        for (m, x, iid, hg) in spec.instances:
            x = np.asarray(x, np.float32).copy()
            if hg == rt.RT_HITGROUP_MODEL:
                if iid % 17 == 3:  # a few rotated, scaled instances (the general transform path)
                    x = scenes._rot_scale((0.2, 1.0, 0.1), 11.0 * k + iid, (1.0, 1.0 + 0.05 * k, 1.0),
                                          (float(x[3]), float(x[7]), float(x[11])))
                else:
                    x[3] += 0.15 * k * ((iid % 3) - 1)
                    x[11] -= 0.1 * k * ((iid % 5) - 2)
            inst.append((m, x, iid, hg))
        c.tlas_build(inst, update_only=True)
        walls.append(c.tlas_build_wall_ms())
        out = torch.empty((spec.height, spec.width, 4), dtype=torch.uint8, device="cuda")
        c.dispatch(spec.width, spec.height, out, None, stream=streams[k % 3].cuda_stream)
        sk = scenes.SceneSpec(**{**spec.__dict__})
        sk.instances = inst
        outs.append(out)
        specs.append(sk)
    torch.cuda.synchronize()
    for k, (out, sk) in enumerate(zip(outs, specs)):
        o8, _, _ = oracle.Scene(sk).render_spec(sk, nthreads=16, want_float=False, schedule=1)
        assert np.array_equal(out.cpu().numpy(), o8), f"frame {k}"
    assert len({o.cpu().numpy().tobytes() for o in outs}) == len(outs)  # every frame saw its own scene
    assert max(walls) > 0.0
    c.close()


def test_rejected_tlas_build_keeps_scene():
    """A TLAS build rejected by validation touches nothing: the previous scene still renders. (A
    build that fails after validation marks the scene stale until a build succeeds: rt_api.cpp.)"""
    spec = scenes.config("C2").with_size(96, 54)
    c, o = load_both(spec)
    bad = list(spec.instances)
    bad[0] = (0, np.zeros(12, np.float32), 0, rt.RT_HITGROUP_MODEL)  # singular transform
    with pytest.raises(rt.RtError):
        c.tlas_build(bad)
    good8, good32 = gpu_render(c, spec)  # validation failed before anything was touched
    o8, o32, _ = o.render_spec(spec, nthreads=4)
    assert_images_equal(good8, good32, o8, o32, "after rejected build")
    c.close()


def test_invalid_arguments_raise():
    c = fresh_ctx()
    v = np.zeros((4, 6), np.float32)
    with pytest.raises(rt.RtError):
        c.blas_build(v)  # non-indexed count not a multiple of 3
    with pytest.raises(rt.RtError):
        c.blas_build(v, np.array([0, 1, 9], np.uint32))  # index out of range
    out = torch.empty((4, 4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(rt.RtError):
        c.dispatch(4, 4, out)  # nothing built yet
    with pytest.raises(rt.RtError):
        c.set_shading(scenes.REFERENCE_LIGHTS[:1], scenes.REFERENCE_MATERIAL, 0, spp=3)
    c.close()


# ------------------------------------------------------------------------------------------
# the C++ host mirror (nv_helpers_hip.hpp) end to end: rt_app == oracle
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,cfg,mode,lights,ranks", [("ref", "REF", "ref", 6, 0), ("grid8", "C4", "lambert_shadow", 2, 0),
                                                         ("ref", "REF", "ref", 6, 1), ("grid8", "C4", "lambert_shadow", 2, 1)])
def test_cpp_host_app_matches_oracle(tmp_path, scene, cfg, mode, lights, ranks):
    """rt_app (the reference application over nv_helpers_hip.hpp) == oracle; with --ranks 1 every frame goes
    through the C-ABI's tiled-frame loop (rt_render_strips over a world-1 RCCL communicator)."""
    import gzip
    import os
    import subprocess
    spec = scenes.config(cfg).with_size(160, 90)
    model = tmp_path / f"{spec.model}.obj"
    model.write_bytes(gzip.open(os.path.join(rt.ASSETS, f"{spec.model}.obj.gz")).read())
    raw = tmp_path / "frame.rgba"
    eye, center, _ = spec.camera
    cmd = [os.path.join(os.path.dirname(rt.LIB_PATH), "rt_app"), "--model", str(model), "--scene", scene,
           "--mode", mode, "--lights", str(lights), "--width", "160", "--height", "90", "--frames", "2",
           "--raw", str(raw), "--eye", *map(str, eye), "--center", *map(str, center)]
    if ranks:
        cmd += ["--ranks", str(ranks), "--rank", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = np.frombuffer(raw.read_bytes(), np.uint8).reshape(90, 160, 4)
    o8, _, _ = oracle.Scene(spec).render_spec(spec, nthreads=4)
    assert np.array_equal(img, o8)


@pytest.mark.parametrize("buttons,dx,dy", [("lmb", 40, -25), ("mmb", -30, 10), ("lmb+alt", 25, 15)])
def test_cpp_host_app_drag_frames(tmp_path, buttons, dx, dy):
    """Interactive camera path: rt_app replays a mouse drag through the C++
    Manipulator (OnButtonDown / OnMouseMove negate the window coordinates, :1206-1234) and dumps
    every frame; each must equal the oracle frame for the view the Python Manipulator reaches
    with the same events."""
    import gzip
    import os
    import subprocess
    W, H, frames = 128, 72, 4
    spec = scenes.config("REF").with_size(W, H)
    model = tmp_path / f"{spec.model}.obj"
    model.write_bytes(gzip.open(os.path.join(rt.ASSETS, f"{spec.model}.obj.gz")).read())
    eye, center, up = spec.camera
    cmd = [os.path.join(os.path.dirname(rt.LIB_PATH), "rt_app"), "--model", str(model), "--scene", "ref",
           "--mode", "ref", "--lights", "6", "--width", str(W), "--height", str(H), "--frames", str(frames),
           "--eye", *map(str, eye), "--center", *map(str, center), "--drag", buttons, str(dx), str(dy),
           "--out-pattern", str(tmp_path / "f%02d.ppm")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = rt.Manipulator()
    m.setWindowSize(W, H)
    m.setLookat(eye, center, up)
    keys = set(buttons.split("+"))
    bits = rt.Manipulator.inputs(**{k: True for k in keys})
    mx, my = W // 2, H // 2
    m.setMousePosition(-mx, -my)
    sc = oracle.Scene(spec)
    views = []
    for f in range(frames):
        if f > 0:
            mx, my = mx + dx, my + dy
            m.mouseMove(-mx, -my, bits)
        views.append(m.getMatrix())
        cb = rt.camera_buffer(m.getMatrix(), W, H)
        o8, _, _ = sc.render(cb, spec.lights, spec.material, spec.mode, spec.spp, W, H, nthreads=4, want_float=False)
        data = (tmp_path / f"f{f:02d}.ppm").read_bytes()
        hdr = f"P6\n{W} {H}\n255\n".encode()
        assert data.startswith(hdr)
        img = np.frombuffer(data[len(hdr):], np.uint8).reshape(H, W, 3)
        assert np.array_equal(img, o8[..., :3]), f"frame {f}"
    assert not np.array_equal(views[0], views[-1])  # the drag moved the camera


@pytest.mark.parametrize("H,W,world", [(99, 33, 4), (99, 36, 3), (7, 4, 2), (1080, 1920, 8), (1083, 1924, 5)])
def test_assemble_kernel_equals_host_twin(H, W, world):
    """4-B path (W % 4 != 0) and the 16-B row-batched path (ragged last row batch, rows < kAsmRows)."""
    from realtimeraytracing_gradproject_amd import distributed as D
    pad = D.padded_rows(H, world)
    g = torch.randint(0, 255, (world, pad, W, 4), dtype=torch.uint8, device="cuda")
    out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the call below runs on the context's own stream, not torch's
    c = fresh_ctx()
    c.assemble_strips(W, H, world, D.STRIP_ROWS, g, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), D.assemble_host(g.cpu().numpy(), H, world))
    c.close()


GOLDEN_SIZES = {"REF": (96, 54), "C1": (64, 64), "C2": (96, 54), "C2F": (96, 54), "C3": (96, 54), "C4": (96, 54),
                "C5": (48, 27), "REFL": (96, 54), "REFLO": (96, 54), "DEGEN": (96, 54)}


@pytest.mark.parametrize("name", list(GOLDEN_SIZES))
def test_gpu_frames_equal_committed_goldens(name):
    import os
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "frames_small.npz"))
    spec = scenes.config(name).with_size(*GOLDEN_SIZES[name])
    c = fresh_ctx()
    scenes.upload(c, spec)
    for sched, key in ((rt.RT_SCHED_PACKET, "stats"), (rt.RT_SCHED_LANE, "stats_lane")):
        c.set_stats(True)
        c.stats_reset()
        g8, g32 = gpu_render(c, spec, schedule=sched)
        s = c.stats()
        assert np.array_equal(g8, gold[f"{name}_rgba8"])
        assert np.array_equal(g32.view(np.uint32), gold[f"{name}_rgba32f"].view(np.uint32))
        assert [s[k] for k in ["primary_rays", "shadow_rays", "aabb_tests", "tri_tests"]] == \
            [int(x) for x in gold[f"{name}_{key}"][:4]]
    c.close()


@pytest.mark.parametrize("case", [0, 1])
def test_stress_cases_schedules_equal_per_ray(case):
    """The stress run's two frames (tests/test_oracle.py _stress_cases: a packet lane taking a float32
    Moller-Trumbore false positive in a box its own slab test rejected): with packet_tri's own-box mask the GPU's
    packet and per-lane frames both equal the oracle's per-ray frame, float32 and RGBA8."""
    from test_oracle import _stress_cases
    name, spec, _ = _stress_cases()[case]
    c, o = load_both(spec)
    o8, o32, _ = o.render_spec(spec, nthreads=16, schedule=1)
    for sched in (rt.RT_SCHED_PACKET, rt.RT_SCHED_LANE):
        g8, g32 = gpu_render(c, spec, schedule=sched)
        assert_images_equal(g8, g32, o8, o32, f"{name} schedule {sched}")
    c.close()


@pytest.mark.parametrize("name,size,nframes", [("C2", (192, 108), 4), ("C4", (200, 101), 3), ("C5", (96, 54), 2),
                                                ("REF", (160, 90), 4), ("C1", (64, 64), 1)])
def test_dispatch_frames_equal_oracle(name, size, nframes):
    """rt_dispatch_frames: n frames in one launch, a camera each, back to back or at a padded stride: every frame
    equals the oracle's frame for its camera (one-sample, 4-spp sample-lane and REF kernels)."""
    base = scenes.config(name).with_size(*size)
    c, o = load_both(base)
    eyes = [(1.5, 1.5, 1.5), (2.2, 1.4, 1.1), (1.1, 1.9, 2.4), (3.0, 2.0, 0.5)]
    specs = []
    for k in range(nframes):
        sp = base.with_size(*size)
        if name in ("C4", "C5"):
            sp.camera = ((18.0 + 2 * k, 14.0 - k, 18.0 - 3 * k), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0))
        else:
            sp.camera = (eyes[k], (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        specs.append(sp)
    W, H = size
    cams = np.stack([sp.camera_buffer().ravel() for sp in specs])
    for pad in (0, 4096):
        stride = W * H * 4 + pad
        buf = torch.full((nframes * stride,), 7, dtype=torch.uint8, device="cuda")
        c.dispatch_frames(W, H, buf.view(nframes, -1), cams, stream=torch.cuda.current_stream().cuda_stream,
                          frame_stride=stride if pad else 0)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        for k, sp in enumerate(specs):
            o8, _, _ = o.render_spec(sp, nthreads=8, want_float=False)
            got = host[k * stride:k * stride + W * H * 4].reshape(H, W, 4)
            assert np.array_equal(got, o8), f"{name} frame {k} pad {pad}"
            if pad:
                assert (host[k * stride + W * H * 4:(k + 1) * stride] == 7).all(), "wrote past the frame"
    with pytest.raises(rt.RtError):
        c.dispatch_frames(W, H, torch.empty((5, H, W, 4), dtype=torch.uint8, device="cuda"))
    c.close()


def test_dispatch_frames_argument_rules():
    """rt_dispatch_frames refuses a frame stride that is not a multiple of 4 bytes (the RGBA8 stores are
    32-bit words), and renders from the cameras it is given on a context whose rt_set_camera was never called (it
    refuses a NULL camera array there)."""
    spec = scenes.config("C2F").with_size(96, 54)
    c = rt.Context(0)
    scenes.upload(c, spec)
    W, H = spec.width, spec.height
    cams = spec.camera_buffer().reshape(1, 64)
    buf = torch.zeros((2 * W * H * 4 + 8,), dtype=torch.uint8, device="cuda")
    with pytest.raises(rt.RtError):
        c.dispatch_frames(W, H, buf.view(1, -1), cams, stream=torch.cuda.current_stream().cuda_stream,
                          frame_stride=W * H * 4 + 2)
    c.close()
    # a context set up without rt_set_camera: the launch's own camera array is enough
    c2 = rt.Context(0)
    scenes.upload(c2, spec, camera=False)
    out = torch.zeros((1, H, W, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(rt.RtError):
        c2.dispatch_frames(W, H, out, None, stream=torch.cuda.current_stream().cuda_stream)
    c2.dispatch_frames(W, H, out, cams, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o8, _, _ = oracle.Scene(spec).render_spec(spec, nthreads=8, want_float=False)
    assert np.array_equal(out[0].cpu().numpy(), o8)
    c2.close()
