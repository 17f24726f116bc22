"""numpy restatements of the G-buffer's motion plane (rt_gbuffer_motion.motion, rt_host_motion_vectors,
rt_host_motion_project), written from the definition in include/rt_api.h: no GPU, no library.

float32, operation by operation (every numpy float32 operation rounds once, numpy never fuses a multiply with an add):

  * object point   P = (p1 u + p2 v) + p0 ((1 - u) - v): the interpolated normal's vertex order and weights, on the
    current and on the previous vertex positions;
  * world point    a 3x4 row-major transform, each row summed left to right: ((m0 x + m1 y) + m2 z) + m3;
  * clip           mul(projection, mul(view, (P, 1))), HLSL's mul(M, v) on XMMATRIX memory: r_i = ((mem[i] v0 +
    mem[4 + i] v1) + mem[8 + i] v2) + mem[12 + i] v3; view = cb[0..15], projection = cb[16..31];
  * screen         x = ((clip.x / clip.w + 1) 0.5) W, y = ((1 - clip.y / clip.w) 0.5) H, in pixels;
  * entry          (x_prev - x_cur, y_prev - y_cur, w_prev, w_cur), the first two +inf where w_prev <= 0.

float64: the same chain with numpy's matrix products, an independent statement of what the plane means.
"""
import numpy as np

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


def vertex_ids(indices, prim):
    prim = np.asarray(prim, np.int64)
    if indices is None:
        return 3 * prim, 3 * prim + 1, 3 * prim + 2
    idx = np.asarray(indices, np.int64).ravel()
    return idx[3 * prim], idx[3 * prim + 1], idx[3 * prim + 2]


def object_points_f32(vertices, indices, prim, uv):
    pos = np.asarray(vertices, F)[:, :3]
    uv = np.asarray(uv, F).reshape(-1, 2)
    i0, i1, i2 = vertex_ids(indices, prim)
    u, v = uv[:, 0], uv[:, 1]
    bz = (F(1.0) - u) - v
    return (pos[i1] * u[:, None] + pos[i2] * v[:, None]) + pos[i0] * bz[:, None]


def xform_f32(m, p):
    m = IDENTITY if m is None else np.asarray(m, F).ravel()
    return np.stack([((m[4 * r] * p[:, 0] + m[4 * r + 1] * p[:, 1]) + m[4 * r + 2] * p[:, 2]) + m[4 * r + 3]
                     for r in range(3)], axis=1)


def _mul4(mem, v):
    return [((mem[i] * v[0] + mem[4 + i] * v[1]) + mem[8 + i] * v[2]) + mem[12 + i] * v[3] for i in range(4)]


def screen_f32(cb, p, width, height):
    """-> x, y, w of world points p (n, 3) under the camera buffer cb."""
    cb = np.asarray(cb, F).ravel()
    one = np.ones(p.shape[0], F)
    clip = _mul4(cb[16:32], _mul4(cb[0:16], [p[:, 0], p[:, 1], p[:, 2], one]))
    w = clip[3]
    with np.errstate(all="ignore"):  # w = 0: the quotient is inf or NaN, as in the library
        x = ((clip[0] / w + F(1.0)) * F(0.5)) * F(width)
        y = ((F(1.0) - clip[1] / w) * F(0.5)) * F(height)
    return x, y, w


def project_f32(pts_cur, pts_prev, cb, prev_cb, width, height):
    """rt_host_motion_project restated: (n, 4) float32."""
    pc, pp = np.asarray(pts_cur, F).reshape(-1, 3), np.asarray(pts_prev, F).reshape(-1, 3)
    xc, yc, wc = screen_f32(cb, pc, width, height)
    xp, yp, wp = screen_f32(cb if prev_cb is None else prev_cb, pp, width, height)
    with np.errstate(all="ignore"):
        mx, my = xp - xc, yp - yc
    behind = wp <= 0
    return np.stack([np.where(behind, F(np.inf), mx), np.where(behind, F(np.inf), my), wp, wc], axis=1).astype(F)


def vectors_f32(vertices, prev_vertices, indices, o2w, prev_o2w, cb, prev_cb, width, height, prim, uv):
    """rt_host_motion_vectors restated: (n, 4) float32."""
    cur = xform_f32(o2w, object_points_f32(vertices, indices, prim, uv))
    prev = xform_f32(o2w if prev_o2w is None else prev_o2w,
                     object_points_f32(vertices if prev_vertices is None else prev_vertices, indices, prim, uv))
    return project_f32(cur, prev, cb, prev_cb, width, height)


# float64 ------------------------------------------------------------------------------------------
def world_points_f64(vertices, indices, o2w, prim, uv):
    pos = np.asarray(vertices, F)[:, :3].astype(np.float64)
    uv = np.asarray(uv, F).astype(np.float64).reshape(-1, 2)
    i0, i1, i2 = vertex_ids(indices, prim)
    w = 1.0 - uv[:, 0] - uv[:, 1]
    p = pos[i0] * w[:, None] + pos[i1] * uv[:, :1] + pos[i2] * uv[:, 1:]
    m = (IDENTITY if o2w is None else np.asarray(o2w, F)).astype(np.float64).reshape(3, 4)
    return p @ m[:, :3].T + m[:, 3]


def screen_f64(cb, p, width, height):
    cb = np.asarray(cb, F).astype(np.float64)
    view, proj = cb[0:16].reshape(4, 4).T, cb[16:32].reshape(4, 4).T  # memory column j = matrix column j
    clip = (proj @ view @ np.concatenate([p, np.ones((p.shape[0], 1))], axis=1).T).T
    w = clip[:, 3]
    return (clip[:, 0] / w + 1.0) * 0.5 * width, (1.0 - clip[:, 1] / w) * 0.5 * height, w


def vectors_f64(vertices, prev_vertices, indices, o2w, prev_o2w, cb, prev_cb, width, height, prim, uv):
    """(n, 8) float64: mx, my, w_prev, w_cur (no +inf rule: callers filter on w), then the two positions x_cur, y_cur,
    x_prev, y_prev."""
    cur = world_points_f64(vertices, indices, o2w, prim, uv)
    prev = world_points_f64(vertices if prev_vertices is None else prev_vertices, indices,
                            o2w if prev_o2w is None else prev_o2w, prim, uv)
    xc, yc, wc = screen_f64(cb, cur, width, height)
    xp, yp, wp = screen_f64(cb if prev_cb is None else prev_cb, prev, width, height)
    return np.stack([xp - xc, yp - yc, wp, wc, xc, yc, xp, yp], axis=1)


def condition(o2w):
    if o2w is None:
        return 1.0
    return float(np.linalg.cond(np.asarray(o2w, np.float64).reshape(3, 4)[:, :3]))
