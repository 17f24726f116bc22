"""numpy restatements of the G-buffer's normal plane (rt_gbuffer.normal, rt_host_shading_normals): no GPU, no library.

float32, operation by operation in the library's pinned order (every numpy float32 operation rounds once, and numpy
never fuses a multiply with an add):

  * dot(a, b)    = (ax bx + ay by) + az bz
  * normalize(v) = v * (1 / sqrt(dot(v, v)))
  * model group  (CalculateInterpolatedWorldNormal, Hit.hlsl:67-81): the normals of the triangle's vertices 1, 2, 0
    against (u, v, (1 - u) - v), summed left to right, normalised, through the normal matrix, normalised again;
  * plane group  (Hit.hlsl:218-222): normalize(cross(p1 - p0, p2 - p0)) through the normal matrix, not renormalised;
  * the normal matrix transpose(inverse(upper 3x3)) as rt_tlas_build derives it: the cofactor inverse in double,
    each entry (cofactor * (1 / det)) rounded to float32.

float64: the same formulas from the mesh data with numpy's own inverse and norms — an independent statement of what
the planes mean, which the float32 results must approach to within float32's rounding.
"""
import numpy as np

F = np.float32
MODEL, PLANE = 0, 2  # RT_HITGROUP_MODEL, RT_HITGROUP_PLANE


def vertex_ids(indices, prim):
    prim = np.asarray(prim, np.int64)
    if indices is None:
        return 3 * prim, 3 * prim + 1, 3 * prim + 2
    idx = np.asarray(indices, np.int64).ravel()
    return idx[3 * prim], idx[3 * prim + 1], idx[3 * prim + 2]


def normal_matrix(o2w):
    """9 float32, row-major: transpose(inverse(upper 3x3)) of the 3x4 row-major object-to-world (None: identity)."""
    if o2w is None:
        return np.eye(3, dtype=F).ravel()
    x = np.asarray(o2w, F).ravel().astype(np.float64)
    m = [x[0], x[1], x[2], x[4], x[5], x[6], x[8], x[9], x[10]]
    c00 = m[4] * m[8] - m[5] * m[7]
    c01 = m[5] * m[6] - m[3] * m[8]
    c02 = m[3] * m[7] - m[4] * m[6]
    det = m[0] * c00 + m[1] * c01 + m[2] * c02
    assert det != 0.0, "singular transform"
    r = 1.0 / det
    inv = [c00 * r, (m[2] * m[7] - m[1] * m[8]) * r, (m[1] * m[5] - m[2] * m[4]) * r,
           c01 * r, (m[0] * m[8] - m[2] * m[6]) * r, (m[2] * m[3] - m[0] * m[5]) * r,
           c02 * r, (m[1] * m[6] - m[0] * m[7]) * r, (m[0] * m[4] - m[1] * m[3]) * r]
    return np.array([inv[j * 3 + i] for i in range(3) for j in range(3)], np.float64).astype(F)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize(v):
    inv = F(1.0) / np.sqrt(_dot(v, v))
    return v * inv[:, None]


def _mat3(m, d):
    return np.stack([(m[0] * d[:, 0] + m[1] * d[:, 1]) + m[2] * d[:, 2],
                     (m[3] * d[:, 0] + m[4] * d[:, 1]) + m[5] * d[:, 2],
                     (m[6] * d[:, 0] + m[7] * d[:, 1]) + m[8] * d[:, 2]], axis=1)


def normals_f32(vertices, indices, o2w, hit_group, prim, uv):
    """(n, 4) float32, w = 0: rt_host_shading_normals restated."""
    vtx = np.asarray(vertices, F)
    uv = np.asarray(uv, F).reshape(-1, 2)
    i0, i1, i2 = vertex_ids(indices, prim)
    m = normal_matrix(o2w)
    with np.errstate(all="ignore"):  # a zero-area triangle's face normal is 0 * inf, as in the library
        if hit_group == PLANE:
            p0, p1, p2 = vtx[i0, :3], vtx[i1, :3], vtx[i2, :3]
            a, b = p1 - p0, p2 - p0
            cr = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                           a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
            n = _mat3(m, _normalize(cr))
        else:
            n0, n1, n2 = vtx[i1, 3:6], vtx[i2, 3:6], vtx[i0, 3:6]
            u, v = uv[:, 0], uv[:, 1]
            bz = (F(1.0) - u) - v
            s = (n0 * u[:, None] + n1 * v[:, None]) + n2 * bz[:, None]
            n = _normalize(_mat3(m, _normalize(s)))
    out = np.zeros((n.shape[0], 4), F)
    out[:, :3] = n
    return out


def normals_f64(vertices, indices, o2w, hit_group, prim, uv):
    """(n, 3) float64: the same normals from the mesh data, every step in double with numpy's own linear algebra."""
    vtx = np.asarray(vertices, F).astype(np.float64)
    uv = np.asarray(uv, F).astype(np.float64).reshape(-1, 2)
    i0, i1, i2 = vertex_ids(indices, prim)
    L = np.eye(3) if o2w is None else np.asarray(o2w, F).astype(np.float64).reshape(3, 4)[:, :3]
    M = np.linalg.inv(L).T
    if hit_group == PLANE:
        n = np.cross(vtx[i1, :3] - vtx[i0, :3], vtx[i2, :3] - vtx[i0, :3])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        return n @ M.T
    w = 1.0 - uv[:, 0] - uv[:, 1]
    n = vtx[i1, 3:6] * uv[:, :1] + vtx[i2, 3:6] * uv[:, 1:] + vtx[i0, 3:6] * w[:, None]
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = n @ M.T
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def condition(o2w):
    if o2w is None:
        return 1.0
    return float(np.linalg.cond(np.asarray(o2w, np.float64).reshape(3, 4)[:, :3]))


def lambert_primary_f32(normal, t, origin, direction, light):
    """RT_SHADE_PRIMARY's colour of a model-group hit under ONE light from the G-buffer's planes, in float32 in the
    kernel's order: P = O + D t, L = normalize(light - P), c = max(0, dot(-n, L)) (a sum over one light, / 1)."""
    n = -np.asarray(normal, F)[:, :3]
    P = np.asarray(origin, F) + np.asarray(direction, F) * np.asarray(t, F)[:, None]
    L = _normalize(np.asarray(light, F)[None, :] - P)
    nl = _dot(n, L)
    c = np.where(nl > 0, F(0.0) + nl * F(1.0), F(0.0)).astype(F)
    return c / F(1.0)
