"""The AO filter (rt_denoise_guide, rt_ao_accumulate, rt_ao_atrous; include/rt_api.h) restated in numpy float32, from
the header's text alone: every operation is one float32 numpy operation (correctly rounded, as IEEE requires of + - * /
and sqrt), in the header's order, and minf / maxf are the header's comparisons, so the host twins must equal it bit for
bit. Also the synthetic planes the CPU and GPU tests share.

Planes are flat, row-major: entry y * W + x."""
import numpy as np

F = np.float32
BIG = F(3.402823466e+38)
H5 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], F)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _minf(a, b):
    return np.where(a < b, a, b).astype(F)


def _maxf(a, b):
    return np.where(a > b, a, b).astype(F)


def guide(normal, depth):
    """normal (n, 4), depth (n,) -> guide (n, 4)."""
    normal = np.asarray(normal, F).reshape(-1, 4)
    z = np.asarray(depth, F).ravel()
    x, y, w = normal[:, 0], normal[:, 1], normal[:, 2]
    with np.errstate(all="ignore"):
        d = _dot(x, y, w, x, y, w)
        valid = (np.abs(x) <= BIG) & (np.abs(y) <= BIG) & (np.abs(w) <= BIG) & (d <= BIG) & (d > 0) & (z <= BIG) & (z > 0)
        inv = F(1.0) / np.sqrt(d)
        out = np.stack([x * inv, y * inv, w * inv, z], axis=1).astype(F)
    out[~valid] = 0.0
    return out


def accumulate(W, H, ao_cur, motion, guide_cur, ao_prev=None, hist_prev=None, guide_prev=None, max_history=32,
               depth_tol=0.02, normal_cos=0.9):
    """-> ao_out, hist_out, taps (n,) int: the taps with a non-zero weight of a pixel that seeks history (0 where it
    does not), accepted (n,) int: how many of them were accepted."""
    n = W * H
    cur = np.asarray(ao_cur, F).ravel()
    m = np.asarray(motion, F).reshape(n, 4)
    g = np.asarray(guide_cur, F).reshape(n, 4)
    yy, xx = np.divmod(np.arange(n), W)
    surface = g[:, 3] != 0
    sw, sa, sh = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    taps, accepted = np.zeros(n, int), np.zeros(n, int)
    if ao_prev is not None:
        ap, hp = np.asarray(ao_prev, F).ravel(), np.asarray(hist_prev, F).ravel()
        q = np.asarray(guide_prev, F).reshape(n, 4)
        tol, ncos = F(depth_tol), F(normal_cos)
        with np.errstate(all="ignore"):
            fx, fy = xx.astype(F) + m[:, 0], yy.astype(F) + m[:, 1]
            seek = surface & (np.abs(m[:, 0]) <= BIG) & (np.abs(m[:, 1]) <= BIG) & (m[:, 2] > 0)
            seek &= (fx > F(-1.0)) & (fx < F(W)) & (fy > F(-1.0)) & (fy < F(H))
            fx, fy = np.where(seek, fx, F(0)), np.where(seek, fy, F(0))
            xf, yf = np.floor(fx), np.floor(fy)
            tx, ty = fx - xf, fy - yf
            x0, y0 = xf.astype(int), yf.astype(int)
            lim = tol * m[:, 2]
            for k in range(4):
                dx, dy = k & 1, k >> 1
                w = ((tx if dx else F(1.0) - tx) * (ty if dy else F(1.0) - ty)).astype(F)
                px, py = x0 + dx, y0 + dy
                live = seek & (w != 0)
                taps += live
                inside = live & (px >= 0) & (py >= 0) & (px < W) & (py < H)
                t = np.where(inside, py * W + px, 0)
                qt = q[t]
                ok = inside & (qt[:, 3] != 0) & ~(np.abs(qt[:, 3] - m[:, 2]) > lim)
                ok &= ~(_dot(g[:, 0], g[:, 1], g[:, 2], qt[:, 0], qt[:, 1], qt[:, 2]) < ncos)
                accepted += ok
                sw = np.where(ok, sw + w, sw).astype(F)
                sa = np.where(ok, sa + w * ap[t], sa).astype(F)
                sh = np.where(ok, sh + w * hp[t], sh).astype(F)
    with np.errstate(all="ignore"):
        blend = surface & (sw >= F(0.01))
        a = sa / sw
        cnt = _minf(sh / sw + F(1.0), F(max_history))
        ao = np.where(blend & (cnt != F(1.0)), a + (F(1.0) / cnt) * (cur - a), cur).astype(F)
        hist = np.where(blend, cnt, np.where(surface, F(1.0), F(0.0))).astype(F)
    return ao, hist, taps, accepted


def atrous_iteration(W, H, s, src, g, depth_tol, normal_cos):
    n = W * H
    yy, xx = np.divmod(np.arange(n), W)
    surface = g[:, 3] != 0
    tol, ncos = F(depth_tol), F(normal_cos)
    sw, sa = np.zeros(n, F), np.zeros(n, F)
    with np.errstate(all="ignore"):
        zden = (tol * g[:, 3]) * F(s)
        nden = F(1.0) - ncos
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = H5[dy + 2] * H5[dx + 2]
                px, py = xx + dx * s, yy + dy * s
                inside = (px >= 0) & (py >= 0) & (px < W) & (py < H)
                t = np.where(inside, py * W + px, 0)
                q = g[t]
                if dx == 0 and dy == 0:
                    ok, w = inside, np.full(n, k, F)
                else:
                    ok = inside & (q[:, 3] != 0)
                    wz = _maxf(F(0.0), F(1.0) - np.abs(q[:, 3] - g[:, 3]) / zden)
                    wn = _minf(F(1.0), _maxf(F(0.0), (_dot(g[:, 0], g[:, 1], g[:, 2], q[:, 0], q[:, 1], q[:, 2]) - ncos)
                                             / nden))
                    e = wz * wn
                    w = (k * (e * e)).astype(F)
                sw = np.where(ok, sw + w, sw).astype(F)
                sa = np.where(ok, sa + w * src[t], sa).astype(F)
        out = sa / sw
    return np.where(surface, out, src).astype(F)


def atrous(W, H, ao_in, guide_plane, iterations=3, depth_tol=0.02, normal_cos=0.9):
    g = np.asarray(guide_plane, F).reshape(W * H, 4)
    v = np.asarray(ao_in, F).ravel()
    for k in range(iterations):
        v = atrous_iteration(W, H, 1 << k, v, g, depth_tol, normal_cos)
    return v


def classes(guide_cur, taps, accepted):
    """Of the pixels with a surface: how many had all their non-zero taps accepted, some, none -> (valid, all, some,
    none)."""
    v = np.asarray(guide_cur, F).reshape(-1, 4)[:, 3] != 0
    full = v & (taps > 0) & (accepted == taps)
    none = v & (accepted == 0)
    return int(v.sum()), int(full.sum()), int((v & ~full & ~none).sum()), int(none.sum())


SIZES = [(1, 1), (3, 2), (37, 21), (70, 67)]  # 70 x 67: all +-32 taps of step 16 in frame for some pixels, none for others
DEPTH_TOL, NORMAL_COS = 0.02, 0.9

_SYN = {}


def synthetic(W, H, seed=0):
    """Two frames' worth of planes that exercise every branch (shared, read-only: callers copy before they modify).
    Three vertical bands with depth noise of 0.3 x, 1.5 x and 10 x depth_tol and normal jitter to match, so that a
    band's reprojection taps are all, partly and hardly ever accepted; random unit and non-unit normals; 10 % of the
    pixels invalid (zero, NaN, inf, overflowing normals, depth <= 0); motion uniform in +-3 px, 10 % of it +inf, and
    whatever falls outside the frame near the edges."""
    key = (W, H, seed)
    if key in _SYN:
        return _SYN[key]
    rng = np.random.default_rng(1000 * seed + 7 * W + H)
    n = W * H
    yy, xx = np.divmod(np.arange(n), W)
    band = np.minimum(3 * xx // max(W, 1), 2)
    base = np.array([0.2, 0.5, 1.0])
    base /= np.linalg.norm(base)
    jitter = np.array([0.02, 0.35, 1.5])[band]
    noise = np.array([0.3, 1.5, 10.0])[band] * DEPTH_TOL
    z0 = 5.0

    def frame():
        nrm = np.zeros((n, 4), F)
        v = base + jitter[:, None] * rng.uniform(-1, 1, (n, 3))
        scale = np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.05, 20.0, n))  # unit (nearly) and non-unit
        nrm[:, :3] = (v / np.linalg.norm(v, axis=1)[:, None] * scale[:, None]).astype(F)
        depth = (z0 * (1.0 + noise * rng.uniform(-1, 1, n))).astype(F)
        bad = rng.random(n) < 0.10
        kind = rng.integers(0, 6, n)
        nrm[bad & (kind == 0), :3] = 0.0
        nrm[bad & (kind == 1), 1] = np.nan
        nrm[bad & (kind == 2), 0] = np.inf
        nrm[bad & (kind == 3), :3] = F(3e38)  # finite components, dot overflows
        depth[bad & (kind == 4)] = 0.0
        depth[bad & (kind == 5)] = -1.0
        depth[bad & (kind == 5) & (rng.random(n) < 0.5)] = np.inf
        return nrm, depth

    nrm_cur, w_cur = frame()
    nrm_prev, w_prev_plane = frame()
    motion = np.zeros((n, 4), F)
    motion[:, :2] = rng.uniform(-3, 3, (n, 2)).astype(F)
    whole = rng.random(n) < 0.15  # whole-pixel motion: zero-weight taps
    motion[whole, :2] = rng.integers(-2, 3, (int(whole.sum()), 2)).astype(F)
    gone = rng.random(n) < 0.10
    motion[gone, :2] = np.inf
    motion[:, 2] = z0
    motion[gone & (rng.random(n) < 0.5), 2] = -1.0  # behind the previous camera: w_prev <= 0 is written too
    motion[:, 3] = w_cur
    out = dict(W=W, H=H, normal_cur=nrm_cur, normal_prev=nrm_prev, depth_prev=w_prev_plane, motion=motion,
               ao_cur=(rng.random(n) < 0.6).astype(F), ao_prev=rng.random(n).astype(F),
               hist_prev=rng.integers(1, 40, n).astype(F))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _SYN[key] = out
    return out
