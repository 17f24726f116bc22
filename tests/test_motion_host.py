"""The G-buffer's motion plane on the host (no GPU): rt_host_motion_vectors and rt_host_motion_project run the two
stages the motion kernels run (rt_device.hpp: motion_object_points, motion_entry), so pinning them here — bit for bit
to a float32 numpy restatement written from the header's definition, to float32 rounding against an independent
float64 one, and to RayGen's own rays for the screen convention — pins what the kernels write;
tests/test_gpu_motion.py then only has to show that the kernels equal these functions."""
import ctypes

import numpy as np
import pytest

import realtimeraytracing_gradproject_amd as rt
from realtimeraytracing_gradproject_amd import scenes

import oracle
import motion_reference as ref
from test_gbuffer_host import XFORMS, bits_equal, meshes, samples

N = 2000
W, H = 640, 360
ZNEAR = 0.1
W_FLOOR, W_EXTENT = 10 * ZNEAR, 50.0  # view depths the rounding bounds are stated for

# the previous frame's transform of each of test_gbuffer_host.py's six: a frame's worth of motion
PREV_XFORMS = {
    "identity": scenes.translation(0.1, -0.05, 0.2),
    "translation": scenes.translation(-5.2, 0.25, 4.9),
    "mirror": np.array([-1, 0, 0, 2.1, 0, 1, 0, 0.4, 0, 0, 1, -3.0], np.float32),
    "scale": np.array([1.45, 0, 0, 0, 0, 0.62, 0, 1.05, 0, 0, 1.0, 0.1], np.float32),
    "rot_scale": scenes._rot_scale((1, 2, 0.5), 30.0, (1.5, 0.6, 1.0), (5.9, 1.0, -2.1)),
    "rot_mirror_scale": scenes._rot_scale((0.3, 1, -0.2), 121.0, (-0.4, 1.9, 0.7), (0.1, 0.5, 6.0)),
}

EYE, CENTER, UP = (7.0, 5.0, 9.0), (0.2, 1.3, 0.0), (0.0, 1.0, 0.0)


def manipulated(inputs, dx, dy):
    """(previous, current) camera buffers: the manipulator at the look-at, then after one mouse step."""
    cam = rt.Manipulator()
    cam.setWindowSize(W, H)
    cam.setLookat(EYE, CENTER, UP)
    before = rt.camera_buffer(cam.getMatrix(), W, H)
    cam.setMousePosition(W // 2, H // 2)
    cam.mouseMove(W // 2 + dx, H // 2 + dy, inputs)
    after = rt.camera_buffer(cam.getMatrix(), W, H)
    assert (before != after).any()
    return before, after


def camera_pairs():
    return {"orbit": manipulated(rt.Manipulator.inputs(lmb=True), 12, -7),
            "dolly": manipulated(rt.Manipulator.inputs(rmb=True), 0, 25)}


def displaced(vertices):
    """The previous frame's vertices: a smooth displacement of the positions (normals untouched)."""
    v = np.array(vertices, np.float32, copy=True)
    p = v[:, :3].astype(np.float64)
    v[:, 0] += (0.05 * np.sin(1.3 * p[:, 1] + 0.4)).astype(np.float32)
    v[:, 1] += (0.04 * np.cos(0.9 * p[:, 2] - 0.2)).astype(np.float32)
    v[:, 2] += (0.03 * np.sin(1.1 * p[:, 0] + 1.0)).astype(np.float32)
    return v


def cases():
    out = []
    pairs = camera_pairs()
    for mk, (mname, mesh) in enumerate(meshes().items()):
        prev_v = displaced(mesh[0])
        for xk, (xname, x) in enumerate(XFORMS.items()):
            for ck, (cname, (pcb, cb)) in enumerate(pairs.items()):
                out.append((f"{mname}-{xname}-{cname}", mesh, prev_v, x, PREV_XFORMS[xname], cb, pcb,
                            1000 + 100 * mk + 10 * xk + ck))
    return out


def library(mesh, prev_v, x, px, cb, pcb, prim, uv):
    return rt.host_motion_vectors(mesh[0], mesh[1], prim, uv, cb, W, H, prev_vertices=prev_v, object_to_world=x,
                                  prev_object_to_world=px, prev_camera=pcb)


def restated(mesh, prev_v, x, px, cb, pcb, prim, uv):
    return ref.vectors_f32(mesh[0], prev_v, mesh[1], x, px, cb, pcb, W, H, prim, uv)


def test_bit_equal_to_float32_restatement():
    """Teapot, degenerate soup and plane under six current and six previous transforms, displaced previous vertices,
    an orbit and a dolly step of the camera, 2,000 random (prim, u, v) each with the corner and edge barycentrics:
    every float of rt_host_motion_vectors equals the restatement's, and rt_host_motion_project the projection stage's."""
    finite = 0
    for name, mesh, prev_v, x, px, cb, pcb, seed in cases():
        prim, uv = samples(mesh, seed)
        got = library(mesh, prev_v, x, px, cb, pcb, prim, uv)
        want = restated(mesh, prev_v, x, px, cb, pcb, prim, uv)
        ok = bits_equal(got, want).all(axis=1)
        assert ok.all(), (f"{name}: {int((~ok).sum())} of {N} differ, first {int(np.nonzero(~ok)[0][0])}: "
                          f"{got[~ok][0]} vs {want[~ok][0]}")
        cur = ref.xform_f32(x, ref.object_points_f32(mesh[0], mesh[1], prim, uv))
        prev = ref.xform_f32(px, ref.object_points_f32(prev_v, mesh[1], prim, uv))
        proj = rt.host_motion_project(cur, prev, cb, pcb, W, H)
        assert bits_equal(proj, want).all(), f"{name}: rt_host_motion_project differs from the projection stage"
        finite += int(np.isfinite(got).all(axis=1).sum())
    assert finite > 0.75 * N * len(cases())  # the plane mesh reaches behind the cameras (+inf there), nothing else does


def test_identical_inputs_give_exact_zeros():
    """The same vertices, transform and camera for both frames (given explicitly, and as the NULL defaults): mx and
    my are exactly 0.0 and w_prev == w_cur bitwise, wherever the point is in front of the camera."""
    front = 0
    for name, mesh, _, x, _, cb, _, seed in cases():
        prim, uv = samples(mesh, seed)
        for got in (library(mesh, mesh[0], ref.IDENTITY if x is None else x, ref.IDENTITY if x is None else x, cb, cb,
                            prim, uv),
                    library(mesh, None, x, None, cb, None, prim, uv)):
            assert (got[:, 2].view(np.uint32) == got[:, 3].view(np.uint32)).all(), name
            ahead = got[:, 3] > 0
            assert (got[ahead, :2].view(np.uint32) == 0).all(), f"{name}: a non-zero motion of an unchanged point"
            assert np.isposinf(got[~ahead, :2]).all()
            front += int(ahead.sum())
    assert front > N * len(cases())  # of 2 N per case


def test_behind_the_previous_camera():
    """The previous camera turned 180 degrees about its eye: what the current camera sees was behind it, so
    mx = my = +inf there, and w_prev is still written."""
    cb = rt.camera_buffer(rt.camera_lookat(EYE, CENTER, UP), W, H)
    back = tuple(2 * e - c for e, c in zip(EYE, CENTER))
    pcb = rt.camera_buffer(rt.camera_lookat(EYE, back, UP), W, H)
    mesh = meshes()["teapot"]
    prim, uv = samples(mesh, 7)
    got = library(mesh, None, None, None, cb, pcb, prim, uv)
    want = restated(mesh, None, None, None, cb, pcb, prim, uv)
    assert bits_equal(got, want).all()
    behind = got[:, 2] <= 0
    assert behind.sum() > N // 2 and (got[behind, 3] > 0).all()
    assert np.isposinf(got[behind, :2]).all() and np.isfinite(got[behind, 2]).all() and (got[behind, 2] < 0).all()
    assert np.isfinite(got[~behind, :2]).all()


# ---- screen convention ---------------------------------------------------------------------------------------------
# Measured with this file (PYTHONPATH=.:tests python tests/test_motion_host.py): the float32 restatement's largest
# |projected position - pixel centre| over ray_points(), in pixels.
CONVENTION_MAX = 5.0354e-4
CONVENTION_BOUND = 8 * CONVENTION_MAX


def ray_points():
    """Points O + t D on RayGen's own rays (oracle.camera_rays) of 4,000 random pixels, both camera buffers of both
    pairs, with view depths between 10 znear and the scenes' extent: -> [(cb, points, pixel centres)]."""
    out = []
    rng = np.random.default_rng(11)
    for pcb, cb in camera_pairs().values():
        for c in (pcb, cb):
            px = rng.integers(0, W, size=4000)
            py = rng.integers(0, H, size=4000)
            px[:4], py[:4] = [0, W - 1, 0, W - 1], [0, 0, H - 1, H - 1]
            rays = oracle.camera_rays(c, W, H, px, py)
            t = rng.uniform(1.5, 45.0, size=px.size).astype(np.float32)
            pts = rays[:, 0:3] + rays[:, 4:7] * t[:, None]
            w = ref.screen_f32(c, pts, W, H)[2]
            keep = (w >= W_FLOOR) & (w <= W_EXTENT)
            out.append((c, pts[keep], np.stack([px[keep] + 0.5, py[keep] + 0.5], axis=1)))
    return out


def convention_deviation(position):
    worst, n = 0.0, 0
    for cb, pts, centre in ray_points():
        x, y = position(cb, pts)
        worst = max(worst, float(np.abs(np.asarray(x, np.float64) - centre[:, 0]).max()),
                    float(np.abs(np.asarray(y, np.float64) - centre[:, 1]).max()))
        n += pts.shape[0]
    return worst, n


def test_projection_inverts_raygen():
    """A point on the camera ray of pixel (px, py) projects to (px + 0.5, py + 0.5): the forward chain is the inverse
    of RayGen's, +x right and +y down, in pixels of the full frame. The library's own projected position is read
    through its motion entry: a previous camera buffer of zeros except view[3][3] = projection[3][3] = 1 gives
    clip = (0, 0, 0, 1), so x_prev = 0.5 W and y_prev = 0.5 H exactly, and the entry is (0.5 W - x_cur, 0.5 H - y_cur);
    each subtraction rounds once, by at most half an ulp of 320 (1.5e-5 px), which the 8 x margin covers."""
    flat = np.zeros(64, np.float32)
    flat[15] = flat[16 + 15] = 1.0

    def through_library(cb, pts):
        m = rt.host_motion_project(pts, pts, cb, flat, W, H)
        assert (m[:, 2] == 1.0).all()
        return 0.5 * W - m[:, 0].astype(np.float64), 0.5 * H - m[:, 1].astype(np.float64)

    worst, n = convention_deviation(through_library)
    print(f"largest |projected position - pixel centre| over {n} points: {worst:.4e} px, bound {CONVENTION_BOUND:.4e}")
    assert n > 8000
    assert worst <= CONVENTION_BOUND


# ---- float64 -------------------------------------------------------------------------------------------------------
# Measured with this file (as above): the float32 restatement's largest |mx, my - float64| in pixels over
# well_conditioned_cases() — over every sample at the stated view depths (the plane mesh reaches 20 frame widths off
# screen, where a pixel coordinate of 1.3e4 has an ulp of 1e-3), and over those whose two positions are in the frame.
F32_VS_F64_MAX = 8.4111e-2
F32_VS_F64_MAX_IN_FRAME = 2.2436e-4
BOUND, BOUND_IN_FRAME = 8 * F32_VS_F64_MAX, 8 * F32_VS_F64_MAX_IN_FRAME


def well_conditioned_cases():
    """Instances whose current and previous upper 3x3 have condition number <= 4."""
    return [c for c in cases() if ref.condition(c[3]) <= 4.0 and ref.condition(c[4]) <= 4.0]


def deviation(fn):
    """Largest |mx, my - float64's| over the samples whose two view depths (in float64) are within
    [W_FLOOR, W_EXTENT], and over those of them whose two positions are inside the frame:
    -> (pixels, samples, pixels in the frame, samples in the frame)."""
    worst, n, worst_in, n_in = 0.0, 0, 0.0, 0
    for name, mesh, prev_v, x, px, cb, pcb, seed in well_conditioned_cases():
        prim, uv = samples(mesh, seed)
        want = ref.vectors_f64(mesh[0], prev_v, mesh[1], x, px, cb, pcb, W, H, prim, uv)
        keep = (want[:, 2:4] >= W_FLOOR).all(axis=1) & (want[:, 2:4] <= W_EXTENT).all(axis=1)
        inside = keep & (want[:, 4:8] >= 0).all(axis=1) & (want[:, [4, 6]] <= W).all(axis=1) & \
            (want[:, [5, 7]] <= H).all(axis=1)
        d = np.abs(fn(mesh, prev_v, x, px, cb, pcb, prim, uv).astype(np.float64)[:, :2] - want[:, :2]).max(axis=1)
        worst, n = max(worst, float(d[keep].max())), n + int(keep.sum())
        if inside.any():
            worst_in, n_in = max(worst_in, float(d[inside].max())), n_in + int(inside.sum())
    return worst, n, worst_in, n_in


def test_close_to_float64_restatement():
    """Against the independent float64 restatement, in pixels, on the well-conditioned cases (30 of the 36) and the
    samples in front of both cameras at view depths within [10 znear, 50]; the tighter bound holds where both
    positions are inside the frame."""
    assert len(well_conditioned_cases()) == 30
    lib, n, lib_in, n_in = deviation(library)
    print(f"largest |float32 - float64| motion: library {lib:.4e} px over {n} samples (bound {BOUND:.4e}), "
          f"{lib_in:.4e} px over the {n_in} in the frame (bound {BOUND_IN_FRAME:.4e})")
    assert n > 0.5 * N * 30 and n_in > 2000
    assert lib <= BOUND and lib_in <= BOUND_IN_FRAME


# ---- errors, structure ---------------------------------------------------------------------------------------------
def test_error_paths():
    v = np.ascontiguousarray(scenes._model("teapot")[0])
    i = np.ascontiguousarray(scenes._model("teapot")[1])
    prim = np.array([0, 1], np.uint32)
    uv = np.zeros((2, 2), np.float32)
    out = np.zeros((2, 4), np.float32)
    cb = rt.camera_buffer(rt.camera_lookat(EYE, CENTER, UP), W, H)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def call(**k):
        a = dict(vtx=v, prev=None, vcount=v.shape[0], stride=24, idx=i, icount=i.size, x=None, px=None, cb=cb,
                 pcb=None, w=W, h=H, prims=prim, uv=uv, n=2, out=out)
        a.update(k)
        return rt.lib.rt_host_motion_vectors(P(a["vtx"]), P(a["prev"]), a["vcount"], a["stride"], P(a["idx"]),
                                             a["icount"], P(a["x"]), P(a["px"]), P(a["cb"]), P(a["pcb"]), a["w"],
                                             a["h"], P(a["prims"]), P(a["uv"]), a["n"], P(a["out"]))

    assert call() == rt.RT_OK
    singular = np.array([1, 0, 0, 0, 2, 0, 0, 0, 3, 0, 0, 0], np.float32)
    assert call(x=singular) == rt.RT_OK and call(px=np.zeros(12, np.float32)) == rt.RT_OK  # used as given
    assert call(stride=12) == rt.RT_OK  # positions alone will do (the same bytes, read with another stride)
    assert call(stride=8) == rt.RT_E_INVALID and call(stride=26) == rt.RT_E_INVALID
    assert call(prims=np.array([0, i.size // 3], np.uint32)) == rt.RT_E_INVALID  # one past the last triangle
    assert call(vtx=None) == rt.RT_E_INVALID and call(prims=None) == rt.RT_E_INVALID
    assert call(uv=None) == rt.RT_E_INVALID and call(out=None) == rt.RT_E_INVALID and call(cb=None) == rt.RT_E_INVALID
    assert call(w=0) == rt.RT_E_INVALID and call(h=0) == rt.RT_E_INVALID
    assert call(icount=i.size - 1) == rt.RT_E_INVALID
    assert call(idx=None, icount=0, vcount=v.shape[0] - v.shape[0] % 3 + 1) == rt.RT_E_INVALID
    bad = i.copy()
    bad[5] = v.shape[0]
    assert call(idx=bad) == rt.RT_E_INVALID
    assert call(n=0, prims=None, uv=None, out=None) == rt.RT_OK  # nothing to do

    pts = np.zeros((2, 3), np.float32)
    project = lambda a, b, n, c, w, h, o: rt.lib.rt_host_motion_project(P(a), P(b), n, P(c), None, w, h, P(o))  # noqa: E731
    assert project(pts, pts, 2, cb, W, H, out) == rt.RT_OK
    assert project(None, pts, 2, cb, W, H, out) == rt.RT_E_INVALID and project(pts, None, 2, cb, W, H, out) == rt.RT_E_INVALID
    assert project(pts, pts, 2, None, W, H, out) == rt.RT_E_INVALID and project(pts, pts, 2, cb, W, H, None) == rt.RT_E_INVALID
    assert project(pts, pts, 2, cb, 0, H, out) == rt.RT_E_INVALID and project(pts, pts, 2, cb, W, 0, out) == rt.RT_E_INVALID
    assert project(None, None, 0, cb, W, H, None) == rt.RT_OK
    with pytest.raises(ValueError):
        rt.host_motion_vectors(v, i, prim, uv[:1], cb, W, H)
    with pytest.raises(ValueError):
        rt.host_motion_vectors(v, i, prim, uv, cb, W, H, prev_vertices=v[:-1])
    with pytest.raises(ValueError):
        rt.host_motion_project(pts, pts[:1], cb, None, W, H)
    with pytest.raises(rt.RtError):
        rt.host_motion_vectors(v, i, np.array([i.size // 3], np.uint32), uv[:1], cb, W, H)


def test_python_structure_matches_header():
    assert ctypes.sizeof(rt.rt_gbuffer_motion) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert [f for f, _ in rt.rt_gbuffer_motion._fields_] == ["hits", "uv", "normal", "object", "motion"]
    assert [f for f, _ in rt.rt_gbuffer_motion._fields_][:4] == [f for f, _ in rt.rt_gbuffer._fields_]
    bound = {n for n, _, _ in rt.SIGNATURES}
    assert {"rt_set_motion_history", "rt_dispatch_gbuffer_motion", "rt_host_motion_project",
            "rt_host_motion_vectors"} <= bound
    assert rt.lib.rt_api_version() == 4  # additions only
    # a null context is refused before anything else is looked at (no GPU call)
    g = rt.rt_gbuffer_motion()
    assert rt.lib.rt_dispatch_gbuffer_motion(None, 8, 8, None, 8, ctypes.byref(g), None, None) == rt.RT_E_INVALID
    assert rt.lib.rt_set_motion_history(None, 1) == rt.RT_E_INVALID


if __name__ == "__main__":  # the measurements behind CONVENTION_MAX and F32_VS_F64_MAX
    conv, n = convention_deviation(lambda cb, pts: ref.screen_f32(cb, pts, W, H)[:2])
    print(f"float32 restatement, projected position vs pixel centre over {n} points: {conv:.4e} px; 8 x = {8 * conv:.4e}")
    f32, n, f32_in, n_in = deviation(restated)
    print(f"float32 restatement vs float64 over {len(well_conditioned_cases())} cases: {f32:.4e} px over {n} samples "
          f"(8 x = {8 * f32:.4e}), {f32_in:.4e} px over the {n_in} in the frame (8 x = {8 * f32_in:.4e})")
