"""The fused frame + G-buffer launch on the GPU (rt_dispatch_rays_gbuffer, Context.dispatch_with_gbuffer).

Every comparison is bit for bit, tolerance 0. The expected values always come from the two separate launches on the same
context: the frame from rt_dispatch_rays (Context.dispatch, pinned to the oracle by tests/test_gpu_parity.py) and the
five planes from rt_dispatch_gbuffer_motion (pinned by tests/test_gpu_gbuffer.py and tests/test_gpu_motion.py). The fused
launch is never its own reference.

Shapes, fills and guard regions are tests/test_gpu_gbuffer.py's: 37 x 21 (partial tiles on both edges, several
workgroups) and 1 x 1; every output, rgba8 and rgba32f included, is pre-filled with 0xAB bytes and followed by a 64-word
guard region. Motion history is on and the previous camera's eye is displaced (tests/test_gpu_denoise.py's moved_eye),
so the expected motion plane is not all zeros, which is asserted on it.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import realtimeraytracing_gradproject_amd as rt  # noqa: E402
from realtimeraytracing_gradproject_amd import scenes  # noqa: E402

import test_gpu_motion as mt  # noqa: E402  (its helpers; not its tests)
from test_gpu_denoise import moved_eye  # noqa: E402
from test_gpu_gbuffer import FILL, GUARD, H, LANE, PACKET, W, assert_plane, spec_of  # noqa: E402

FRAME = (("rgba8", 1), ("rgba32f", 4))
OUTPUTS = FRAME + mt.PLANES
ALL = mt.ALL
EYE_STEP = (0.3, 0.15, -0.2)
TRAVERSAL = mt.TRAVERSAL
VARIANTS = ["n1", "n1root", "rays2", "alt", "wavetimes", "ldstop", "popcullblas", "popcullstats"]


# REF, REFL and C1 keep the reference camera, which sits inside teapot 0: at 37 x 21 every pixel is a hit (the oracle:
# 777 hits, 0 misses). The cases are their scenes, materials and shade modes seen from outside, so that each frame has
# hits and misses: REFLO's camera for the reference scene (592 hits, 185 misses, instances 0 and 1 on screen: with
# REFL's material the oracle counts 70 reflection rays), C2F's for C1's teapot.
OUTSIDE = {"REF": scenes.config("REFLO").camera, "REFL": scenes.config("REFLO").camera, "C1": scenes.config("C2F").camera}


def case_spec(name, w=W, h=H):
    """The spec of a case: REF is RT_SHADE_REF with reflectivity 0, REFL the same scene with a reflective material,
    C2F RT_SHADE_LAMBERT_SHADOW, C1 RT_SHADE_PRIMARY; one sample per pixel all."""
    spec = spec_of(name, w, h)
    if name in OUTSIDE:
        spec = scenes.SceneSpec(**{**spec.__dict__})
        spec.camera = OUTSIDE[name]
    assert spec.spp == 1
    return spec


def prev_cb_of(spec):
    return moved_eye(spec, EYE_STEP).camera_buffer()


# ---- launches ------------------------------------------------------------------------------------------------------
def alloc(w, h, rows=None, planes=ALL, frame=("rgba8", "rgba32f")):
    """Pre-filled outputs (on torch's current stream), each followed by its guard region."""
    n = (h if rows is None else len(rows)) * w
    return {name: torch.full((n * words + GUARD,), int(FILL.view(np.int32)), dtype=torch.int32, device="cuda")
            for name, words in OUTPUTS if name in planes or name in frame}


def _args(bufs):
    return {name: t[:t.numel() - GUARD] for name, t in bufs.items()}


def _stream(stream):
    return torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream


def launch_fused(c, w, h, bufs, rows=None, stream=None, prev_camera=None):
    """One fused launch into `bufs` (no synchronisation); absent planes are not passed."""
    c.dispatch_with_gbuffer(w, h, rows=rows, stream=_stream(stream), prev_camera=prev_camera, **_args(bufs))


def launch_separate(c, w, h, bufs, rows=None, stream=None, prev_camera=None):
    """rt_dispatch_rays, then rt_dispatch_gbuffer_motion, into `bufs`."""
    a = _args(bufs)
    c.dispatch(w, h, a.pop("rgba8"), a.pop("rgba32f", None), rows=rows, stream=_stream(stream))
    if a:
        c.dispatch_gbuffer_motion(w, h, rows=rows, stream=_stream(stream), prev_camera=prev_camera, **a)


def collect(bufs):
    """-> {output: (n, words) uint32}; the guard regions must still hold the fill."""
    out = {}
    for name, words in OUTPUTS:
        if name in bufs:
            a = bufs[name].cpu().numpy().view(np.uint32)
            assert (a[-GUARD:] == FILL).all(), f"{name}: the guard region after the output was written"
            out[name] = a[:-GUARD].reshape(-1, words)
    return out


def run(launch, c, w, h, rows=None, planes=ALL, frame=("rgba8", "rgba32f"), prev_camera=None):
    bufs = alloc(w, h, rows, planes, frame)
    launch(c, w, h, bufs, rows, prev_camera=prev_camera)
    torch.cuda.synchronize()
    return collect(bufs)


def assert_outputs(got, want, what):
    assert list(got) == list(want), f"{what}: outputs {list(got)} vs {list(want)}"
    for name in got:
        assert_plane(got[name], want[name], f"{what} {name} vs the separate launches")


def assert_fused_equals_separate(c, w, h, what, rows=None, planes=ALL, frame=("rgba8", "rgba32f"), prev_camera=None,
                                 want=None):
    """-> (the fused launch's outputs, the separate launches')."""
    if want is None:
        want = run(launch_separate, c, w, h, rows, planes, frame, prev_camera)
    got = run(launch_fused, c, w, h, rows, planes, frame, prev_camera)
    assert_outputs(got, want, what)
    return got, want


def assert_hits_and_misses(want, what):
    nhit = int((want["hits"][:, 3] == 1).sum())
    assert 0 < nhit < want["hits"].shape[0], f"{what}: {nhit} hits of {want['hits'].shape[0]} pixels"


def counting_dispatch(c, w, h):
    """The device counters of one rt_dispatch_rays (counters switched on for it, then off again)."""
    c.set_stats(True)
    c.stats_reset()
    out8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    c.dispatch(w, h, out8, stream=_stream(None))
    s = c.stats()
    c.set_stats(False)
    return s


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [PACKET, LANE], ids=["packet", "lane"])
@pytest.mark.parametrize("name", ["REF", "REFL", "C2F", "C1", "DEGEN"])
def test_modes_and_schedules(name, schedule):
    spec = case_spec(name)
    prev_cb = prev_cb_of(spec)
    c, _ = mt.history_context(spec)
    with c:
        c.set_schedule(schedule)
        want = run(launch_separate, c, W, H, prev_camera=prev_cb)
        assert_hits_and_misses(want, name)
        assert mt.moving(want) > 0, f"{name}: the expected motion plane is all zeros"
        assert (want["rgba8"] != want["rgba8"][0]).any(), f"{name}: a flat frame"
        if name == "REFL":  # the primary hit record is overwritten by the reflection walks
            assert counting_dispatch(c, W, H)["reflection_rays"] > 0
        assert_fused_equals_separate(c, W, H, name, prev_camera=prev_cb, want=want)


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [PACKET, LANE], ids=["packet", "lane"])
def test_all_miss_and_single_pixel_frames(schedule):
    for name, w, h, nhit in (("AWAY", W, H, 0), ("C2F", 1, 1, 1), ("AWAY", 1, 1, 0)):
        spec = case_spec(name, w, h)
        prev_cb = prev_cb_of(spec)
        c, _ = mt.history_context(spec)
        with c:
            c.set_schedule(schedule)
            _, want = assert_fused_equals_separate(c, w, h, f"{name} {w} x {h}", prev_camera=prev_cb)
            assert int((want["hits"][:, 3] == 1).sum()) == nhit


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [PACKET, LANE], ids=["packet", "lane"])
def test_row_lists_and_single_planes(schedule):
    rows = np.array([20, 3, 3, 11, 0], np.uint32)
    spec = case_spec("DEGEN")
    prev_cb = prev_cb_of(spec)
    c, _ = mt.history_context(spec)
    with c:
        c.set_schedule(schedule)
        full = run(launch_separate, c, W, H, prev_camera=prev_cb)
        want = run(launch_separate, c, W, H, rows, prev_camera=prev_cb)
        for name, words in OUTPUTS:  # the separate launches' row lists are the full frame's rows
            assert_plane(want[name], full[name].reshape(H, W, words)[rows].reshape(-1, words), f"rows {name}")
        assert_hits_and_misses(want, "DEGEN rows")
        assert_fused_equals_separate(c, W, H, "rows", rows, prev_camera=prev_cb, want=want)
        for name, _ in mt.PLANES:
            alone = run(launch_fused, c, W, H, rows, planes=(name,), prev_camera=prev_cb)
            assert list(alone) == ["rgba8", "rgba32f", name]
            for out in alone:
                assert_plane(alone[out], want[out], f"{name} alone: {out}")
        no_float = run(launch_fused, c, W, H, rows, planes=("motion",), frame=("rgba8",), prev_camera=prev_cb)
        assert list(no_float) == ["rgba8", "motion"]
        for out in no_float:
            assert_plane(no_float[out], want[out], f"no rgba32f: {out}")


# 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [PACKET, LANE], ids=["packet", "lane"])
@pytest.mark.parametrize("name", ["REFL", "C2F"])
def test_counters_equal_a_frame(name, schedule):
    spec = case_spec(name)
    prev_cb = prev_cb_of(spec)
    c, _ = mt.history_context(spec)
    with c:
        c.set_schedule(schedule)
        want = run(launch_separate, c, W, H, prev_camera=prev_cb)
        frame = counting_dispatch(c, W, H)
        c.set_stats(True)
        c.stats_reset()
        got = run(launch_fused, c, W, H, prev_camera=prev_cb)
        fused = c.stats()
        c.set_stats(False)
        assert_outputs(got, want, f"{name}, the counting kernels")
    assert len(frame) == 12
    for k in rt.STAT_NAMES:
        assert fused[k] == frame[k], f"{k}: fused {fused[k]}, rt_dispatch_rays {frame[k]}"
    assert frame["primary_rays"] == frame["pixels"] == W * H and frame["dispatches"] == 1
    assert frame["shadow_rays"] > 0 and (name != "REFL" or frame["reflection_rays"] > 0)


# 5 ------------------------------------------------------------------------------------------------------------------
def test_packet_stack_fallback():
    """CHAIN's packet-stack bound is 64 or more: under the default schedule the fused launch runs the per-lane fused
    kernel, as a frame does. Outputs equal, traversal counters the RT_SCHED_LANE launch's."""
    spec = case_spec("CHAIN")
    prev_cb = prev_cb_of(spec)
    c, ids = mt.history_context(spec)
    with c:
        assert c.tlas_info().max_stack + c.blas_info(ids[1]).depth >= 64
        _, want = assert_fused_equals_separate(c, W, H, "CHAIN", prev_camera=prev_cb)
        assert_hits_and_misses(want, "CHAIN")
        c.set_stats(True)
        got = {}
        for schedule in (PACKET, LANE):
            c.set_schedule(schedule)
            c.stats_reset()
            assert_outputs(run(launch_fused, c, W, H, prev_camera=prev_cb), want, f"CHAIN counting, schedule {schedule}")
            got[schedule] = c.stats()
    for k in TRAVERSAL + ("primary_rays", "stack_overflows"):
        assert got[PACKET][k] == got[LANE][k], f"{k}: {got[PACKET][k]} vs {got[LANE][k]}"
    assert got[PACKET]["stack_overflows"] == 0 and got[PACKET]["node_fetches"] > W * H


# 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [PACKET, LANE], ids=["packet", "lane"])
def test_watertight(schedule):
    spec = case_spec("DEGEN")
    prev_cb = prev_cb_of(spec)
    c, _ = mt.history_context(spec)
    with c:
        c.set_schedule(schedule)
        plain = run(launch_separate, c, W, H, prev_camera=prev_cb)
        c.set_triangle_test(rt.RT_TRIANGLE_TEST_WATERTIGHT)
        _, want = assert_fused_equals_separate(c, W, H, "watertight", prev_camera=prev_cb)
        assert (want["uv"] != plain["uv"]).any()  # the two tests differ in their last bits
        for stats in (True, False):
            c.set_stats(stats)
            assert_outputs(run(launch_fused, c, W, H, prev_camera=prev_cb), want, f"watertight, counters {stats}")
        c.set_triangle_test(rt.RT_TRIANGLE_TEST_MOLLER_TRUMBORE)
        assert_outputs(run(launch_fused, c, W, H, prev_camera=prev_cb), plain, "back to Moller-Trumbore")


# 7 ------------------------------------------------------------------------------------------------------------------
def test_tile_balance_and_tile_rows_are_ignored():
    spec = case_spec("C2F")
    prev_cb = prev_cb_of(spec)
    c, _ = mt.history_context(spec)
    with c:
        c.set_tile_balance(0)
        want = run(launch_separate, c, W, H, prev_camera=prev_cb)
        assert_hits_and_misses(want, "C2F")
        for mode in (0, 1, 2, 3, 4, 5):
            c.set_tile_balance(mode)
            for k in range(3):  # the adaptive balance records, plans and uses a list over consecutive frames
                assert_outputs(run(launch_fused, c, W, H, prev_camera=prev_cb), want, f"balance {mode}, launch {k}")
        c.set_tile_balance(0)
        c.set_tile_rows(4)
        assert_outputs(run(launch_fused, c, W, H, prev_camera=prev_cb), want, "tile rows 4")
        c.set_tile_rows(8)
        # a fused launch between two frames of the adaptive balance disturbs nothing
        c.set_tile_balance(1)
        first = run(launch_separate, c, W, H, planes=(), prev_camera=prev_cb)
        before = c.tile_balance_info()
        assert_outputs(run(launch_fused, c, W, H, prev_camera=prev_cb), want, "between two balanced frames")
        assert c.tile_balance_info() == before, "the fused launch touched the tile balance's state"
        third = run(launch_separate, c, W, H, planes=(), prev_camera=prev_cb)
        assert_outputs(third, first, "the frame after the fused launch")
        assert_plane(first["rgba8"], want["rgba8"], "balanced frame")


# 8 ------------------------------------------------------------------------------------------------------------------
def test_tlas_update_between_launches_on_two_streams():
    """Fused launch A on stream 1, a TLAS update that moves the instances, fused launch B on stream 2, no host
    synchronisation in between: each equals the separate launches of its own scene."""
    spec = case_spec("C2F")
    prev_cb = prev_cb_of(spec)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c, ids = mt.history_context(spec)
    with c:
        want_a = run(launch_separate, c, W, H, prev_camera=prev_cb)
        a, b = alloc(W, H), alloc(W, H)
        torch.cuda.synchronize()  # the fills are done; from here on no host wait until both launches are issued
        launch_fused(c, W, H, a, stream=s1, prev_camera=prev_cb)
        c.tlas_build(mt.instances_of(ids, spec, mt.MOVED), update_only=True)
        launch_fused(c, W, H, b, stream=s2, prev_camera=prev_cb)
        torch.cuda.synchronize()
        got_a, got_b = collect(a), collect(b)
        want_b = run(launch_separate, c, W, H, prev_camera=prev_cb)
        c.forget_stream(s1.cuda_stream)
        c.forget_stream(s2.cuda_stream)
    assert_outputs(got_a, want_a, "before the update")
    assert_outputs(got_b, want_b, "after the update")
    assert (want_a["hits"] != want_b["hits"]).any() and (want_a["rgba8"] != want_b["rgba8"]).any()
    assert (want_a["motion"] != want_b["motion"]).any()


# 9 ------------------------------------------------------------------------------------------------------------------
def test_error_cases_write_nothing():
    spec = case_spec("C2F")
    n = W * H
    bufs = {name: torch.full((n * words,), int(FILL.view(np.int32)), dtype=torch.int32, device="cuda")
            for name, words in OUTPUTS}
    g = rt.rt_gbuffer_motion(*[bufs[name].data_ptr() for name, _ in mt.PLANES])
    no_motion = rt.rt_gbuffer_motion(*[bufs[name].data_ptr() for name, _ in mt.PLANES[:4]], None)
    bad_row = (ctypes.c_uint32 * 2)(0, H)

    def call(c, w=W, h=H, rows=None, nrows=H, out=g, rgba8=bufs["rgba8"].data_ptr()):
        return c._lib.rt_dispatch_rays_gbuffer(c._h, w, h, rows, nrows, rgba8, bufs["rgba32f"].data_ptr(),
                                               None if out is None else ctypes.byref(out), None, None)

    def refused(c, status, word, **kw):
        assert call(c, **kw) == status
        msg = c._lib.rt_last_error(c._h)
        assert word in msg and b"rt_dispatch_rays_gbuffer" in msg, msg

    c, ids = mt.history_context(spec)
    with c:
        c.set_shading(spec.lights, spec.material, spec.mode, 4)
        refused(c, rt.RT_E_INVALID, b"spp")
        c.set_shading(spec.lights, spec.material, spec.mode, 1)
        refused(c, rt.RT_E_INVALID, b"null", out=rt.rt_gbuffer_motion())
        refused(c, rt.RT_E_INVALID, b"null", out=None)
        odd = rt.rt_gbuffer_motion(None, None, bufs["normal"].data_ptr() + 4, None, None)
        refused(c, rt.RT_E_INVALID, b"aligned", out=odd)
        refused(c, rt.RT_E_INVALID, b"row", rows=bad_row, nrows=2)
        refused(c, rt.RT_E_INVALID, b"output", rgba8=None)
        refused(c, rt.RT_E_INVALID, b"size", w=0)
        c.blas_refit(ids[0], spec.meshes[0][0])
        refused(c, rt.RT_E_INVALID, b"refit")
        with pytest.raises(ValueError):  # the Python layer checks the element counts
            c.dispatch_with_gbuffer(W, H, bufs["rgba8"], hits=bufs["uv"])
    with rt.Context(0) as c:  # motion history off
        scenes.upload(c, spec)
        refused(c, rt.RT_E_INVALID, b"history")
        assert call(c, out=no_motion) == rt.RT_OK  # the same buffers are fine for a valid call
        torch.cuda.synchronize()
        for name, _ in OUTPUTS:
            a = bufs[name].cpu().numpy().view(np.uint32)
            assert (a == FILL).all() == (name == "motion"), f"{name} after a valid launch without a motion plane"
            bufs[name].fill_(int(FILL.view(np.int32)))
    with rt.Context(0) as c:  # no camera
        scenes.upload(c, spec, camera=False)
        refused(c, rt.RT_E_INVALID, b"camera", out=no_motion)
    with rt.Context(0) as c:  # no rt_set_shading
        ids = [c.blas_build(v, i) for (v, i) in spec.meshes]
        c.tlas_build(mt.instances_of(ids, spec))
        c.set_camera(spec.camera_buffer())
        refused(c, rt.RT_E_INVALID, b"shading", out=no_motion)
    with rt.Context(0) as c:  # no TLAS
        c.set_camera(spec.camera_buffer())
        refused(c, rt.RT_E_INVALID, b"TLAS", out=no_motion)
    torch.cuda.synchronize()
    for name, _ in OUTPUTS:
        assert (bufs[name].cpu().numpy().view(np.uint32) == FILL).all(), f"{name} written by a refused call"


# 10 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", VARIANTS)
def test_variant_libraries(var):
    """Every variant library hosts the fused kernels (DESIGN §3.12 names none that does not). The wavetimes variant's
    packet kernels put their wave clocks where the float image goes, so its float output is left out."""
    path = os.path.join(os.path.dirname(rt.LIB_PATH), "variants", var, "librtamd.so")
    assert os.path.exists(path), f"{path} missing: `make` builds the variants (no fallback)"
    spec = case_spec("DEGEN")
    prev_cb = prev_cb_of(spec)
    frame = ("rgba8",) if var == "wavetimes" else ("rgba8", "rgba32f")
    with rt.Context(0, library=rt._load(path)) as c:
        c.set_motion_history(True)
        scenes.upload(c, spec)
        for schedule in (PACKET, LANE):
            c.set_schedule(schedule)
            want = run(launch_separate, c, W, H, frame=frame, prev_camera=prev_cb)
            assert_hits_and_misses(want, var)
            for stats in (False, True):  # the plain and the counting kernels
                c.set_stats(stats)
                assert_outputs(run(launch_fused, c, W, H, frame=frame, prev_camera=prev_cb), want,
                               f"{var} stats {stats} schedule {schedule}")
        assert c.stats()["stack_overflows"] == 0
