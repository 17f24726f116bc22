"""The temporal upscaler (rt_upscale, rt_camera_jitter, rt_jitter_halton; include/rt_api.h) restated in numpy float32,
from the header's text alone: every operation is one float32 numpy operation (correctly rounded, as IEEE requires of
+ - * /), in the header's order, and minf / maxf are the header's comparisons, so rt_host_upscale must equal it bit for
bit. Also the synthetic planes the CPU and GPU tests share.

Planes are flat, row-major: entry y * width + x."""
from fractions import Fraction

import numpy as np

F = np.float32
BIG = F(3.402823466e+38)
INF = F(np.inf)


def _minf(a, b):
    return np.where(a < b, a, b).astype(F)


def _maxf(a, b):
    return np.where(a > b, a, b).astype(F)


def _pos(X, s, j, n):
    raw = (X.astype(F) + F(0.5)) * s - j
    return raw, _minf(_maxf(raw, F(0.5)), F(n) - F(0.5))


def _cell(u, n):
    return np.clip(np.floor(u).astype(np.int64), 0, n - 1)


def unorm8(c):
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        mid = (c > F(0.0)) & ~(c >= F(1.0))  # NaN is neither: 0
        v = np.where(mid, c * F(255.0) + F(0.5), F(0.0)).astype(F)
    return np.where(c >= F(1.0), 255, v.astype(np.uint32)).astype(np.uint8)


def upscale(w, h, W, H, color_cur, motion_cur, motion_prev=None, color_prev=None, hist_prev=None,
            jitter_cur=(0.0, 0.0), jitter_prev=(0.0, 0.0), max_history=16, depth_tol=0.02):
    """-> color_out (N, 4), hist_out (N,), rgba8 (N, 4) uint8, info: per output pixel, `taps` the bilinear taps with a
    non-zero weight of a pixel that seeks history (0 where it does not), `accepted` how many of them passed, `clamped`
    whether the sample-grid position was clamped at the border, `dilated` whether the dilation chose a non-centre tap,
    `hist_clamped` whether the history clamp changed a channel of a, `blend` whether history was used."""
    n, N = w * h, W * H
    cc = np.asarray(color_cur, F).reshape(n, 4)
    mc = np.asarray(motion_cur, F).reshape(n, 4)
    jcx, jcy, jpx, jpy = F(jitter_cur[0]), F(jitter_cur[1]), F(jitter_prev[0]), F(jitter_prev[1])
    Y, X = np.divmod(np.arange(N), W)
    with np.errstate(all="ignore"):
        sx, sy = F(w) / F(W), F(h) / F(H)
        rx, ux = _pos(X, sx, jcx, w)
        ry, uy = _pos(Y, sy, jcy, h)
        clamped = (rx != ux) | (ry != uy)
        ic, jc = _cell(ux, w), _cell(uy, h)
        sw, conf = np.zeros(N, F), np.zeros(N, F)
        sc = np.zeros((N, 4), F)
        mn, mx = np.full((N, 4), INF, F), np.full((N, 4), -INF, F)
        m = np.zeros((N, 4), F)
        dil, zbest, noncentre = np.zeros(N, bool), np.zeros(N, F), np.zeros(N, bool)
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                i, j = ic + di, jc + dj
                inside = (i >= 0) & (j >= 0) & (i < w) & (j < h)
                t = np.where(inside, j * w + i, 0)
                c, q = cc[t], mc[t]
                dx, dy = (i.astype(F) + F(0.5)) - ux, (j.astype(F) + F(0.5)) - uy
                k = _maxf(F(0.0), F(1.0) - (dx * dx + dy * dy))
                kw = (k * k).astype(F)
                sw = np.where(inside, sw + kw, sw).astype(F)
                sc = np.where(inside[:, None], sc + kw[:, None] * c, sc).astype(F)
                mn = np.where(inside[:, None], _minf(mn, c), mn).astype(F)
                mx = np.where(inside[:, None], _maxf(mx, c), mx).astype(F)
                centre = di == 0 and dj == 0
                if centre:
                    conf = kw
                surf = inside & (q[:, 3] <= BIG) & (q[:, 3] > F(0.0))
                take = inside & np.where(surf, ~dil | (q[:, 3] < zbest), centre & ~dil)
                m = np.where(take[:, None], q, m).astype(F)
                noncentre = np.where(take, not centre, noncentre)
                zbest = np.where(take & surf, q[:, 3], zbest).astype(F)
                dil = dil | surf
        cur = _minf(_maxf(sc / sw[:, None], mn), mx)
        sw2, sh, sa = np.zeros(N, F), np.zeros(N, F), np.zeros((N, 4), F)
        taps, accepted = np.zeros(N, int), np.zeros(N, int)
        if color_prev is not None:
            cp = np.asarray(color_prev, F).reshape(N, 4)
            hp = np.asarray(hist_prev, F).ravel()
            zp = np.asarray(motion_prev, F).reshape(n, 4)[:, 3]
            seek = (np.abs(m[:, 0]) <= BIG) & (np.abs(m[:, 1]) <= BIG) & (m[:, 2] > F(0.0))
            tmx, tmy = m[:, 0] + (jpx - jcx), m[:, 1] + (jpy - jcy)
            fx, fy = X.astype(F) + tmx / sx, Y.astype(F) + tmy / sy
            seek &= (fx > F(-1.0)) & (fx < F(W)) & (fy > F(-1.0)) & (fy < F(H))
            fx, fy = np.where(seek, fx, F(0)), np.where(seek, fy, F(0))
            xf, yf = np.floor(fx), np.floor(fy)
            tx, ty = fx - xf, fy - yf
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            lim = F(depth_tol) * m[:, 2]
            for t4 in range(4):
                ddx, ddy = t4 & 1, t4 >> 1
                wt = ((tx if ddx else F(1.0) - tx) * (ty if ddy else F(1.0) - ty)).astype(F)
                xx, yy = x0 + ddx, y0 + ddy
                live = seek & (wt != 0)
                taps += live
                inside = live & (xx >= 0) & (yy >= 0) & (xx < W) & (yy < H)
                xs, ys = np.where(inside, xx, 0), np.where(inside, yy, 0)
                pi = _cell((xs.astype(F) + F(0.5)) * sx - jpx, w)
                pj = _cell((ys.astype(F) + F(0.5)) * sy - jpy, h)
                z = zp[pj * w + pi]
                ok = inside & (np.abs(z - m[:, 2]) <= lim)
                accepted += ok
                e = ys * W + xs
                sw2 = np.where(ok, sw2 + wt, sw2).astype(F)
                sa = np.where(ok[:, None], sa + wt[:, None] * cp[e], sa).astype(F)
                sh = np.where(ok, sh + wt * hp[e], sh).astype(F)
        blend = sw2 >= F(0.01)
        cnt = np.where(blend, _minf(sh / sw2 + F(1.0), F(max_history)), F(1.0)).astype(F)
        a = sa / sw2[:, None]
        ext = (mx - mn).astype(F)  # an edge pixel (position clamped): the range widened by its extent on either side
        lo = np.where(clamped[:, None], mn - ext, mn).astype(F)
        hi = np.where(clamped[:, None], mx + ext, mx).astype(F)
        ac = _minf(_maxf(a, lo), hi)
        alpha = (conf * (F(1.0) / cnt)).astype(F)
        mixed = (ac + alpha[:, None] * (cur - ac)).astype(F)
        out = np.where((blend & (cnt != F(1.0)))[:, None], mixed, cur).astype(F)
        hist_clamped = blend & np.any(ac != a, axis=1)
    info = dict(taps=taps, accepted=accepted, clamped=clamped, dilated=noncentre, hist_clamped=hist_clamped, blend=blend)
    return out, cnt, unorm8(out), info


def classes(info):
    """Output-pixel counts: all non-zero bilinear taps accepted, some, none; position clamped; dilation off-centre;
    history clamp active."""
    taps, acc = info["taps"], info["accepted"]
    full = (taps > 0) & (acc == taps)
    none = acc == 0
    return dict(all=int(full.sum()), some=int((~full & ~none).sum()), none=int(none.sum()),
                clamped=int(info["clamped"].sum()), dilated=int(info["dilated"].sum()),
                hist_clamped=int(info["hist_clamped"].sum()))


def camera_jitter(cb, W, H, jx, jy):
    """rt_camera_jitter from the header's text: element (row i, column j) of a matrix is float 4 j + i."""
    cb = np.asarray(cb, F).ravel()
    out = cb.copy()
    if jx == 0 and jy == 0:
        return out
    ax, ay = (F(2.0) * F(jx)) / F(W), (F(2.0) * F(jy)) / F(H)
    p, q = cb[16:32], cb[48:64]
    for j in range(4):
        out[16 + 4 * j + 0] = p[4 * j + 0] - ax * p[4 * j + 3]
        out[16 + 4 * j + 1] = p[4 * j + 1] + ay * p[4 * j + 3]
    for i in range(4):
        out[48 + 12 + i] = (q[12 + i] + ax * q[i]) - ay * q[4 + i]
    return out


def halton(index):
    """rt_jitter_halton's closed form: the exact radical inverses of i = index % (3^15 - 1) + 1, each rounded to
    float32 once, minus 0.5 in float32."""
    i = index % 14348906 + 1

    def radical(k, b):
        v, f = Fraction(0), Fraction(1, b)
        while k:
            v += (k % b) * f
            k //= b
            f /= b
        return v

    def f32(fr):  # the float32 nearest to the exact fraction: its terms are below 2^24, so exact in float32, and the
        return F(fr.numerator) / F(fr.denominator)  # IEEE quotient of two exact operands is correctly rounded

    return f32(radical(i, 2)) - F(0.5), f32(radical(i, 3)) - F(0.5)


# render size, display size
SIZES = [((1, 1), (1, 1)), ((1, 1), (4, 4)), ((3, 2), (7, 5)), ((19, 11), (37, 21)), ((37, 21), (37, 21)),
         ((24, 14), (96, 54))]
CLASS_SIZE = ((19, 11), (37, 21))
DEPTH_TOL, MAX_HISTORY = 0.02, 16
JITTER_CUR, JITTER_PREV = (0.3, -0.2), (-0.4, 0.1)

_SYN = {}


def synthetic(w, h, W, H, seed=0):
    """One call's worth of planes that exercise every branch (shared, read-only: callers copy before they modify).
    Current motion: uniform in +-3 render pixels, 15 % whole pixels, 10 % +inf (half of those with w_prev <= 0), and
    whatever falls outside the frame near the edges; w_prev 5 everywhere else. Current depth (motion .w): 5 with 20 %
    noise, so the dilation mostly picks a neighbour, 10 % of it 0, negative, inf or NaN. Previous depth: 5 with noise
    of 0.3 x, 1.5 x and 10 x depth_tol in three vertical bands, so that a band's bilinear taps are all, partly and
    hardly ever accepted, 5 % of it inf or NaN. Colours uniform in [0, 1) (alpha too), history lengths 1 .. 40."""
    key = (w, h, W, H, seed)
    if key in _SYN:
        return _SYN[key]
    rng = np.random.default_rng(1000 * seed + 131 * w + 17 * h + 7 * W + H)
    n, N = w * h, W * H
    z0 = 5.0
    motion = np.zeros((n, 4), F)
    motion[:, :2] = rng.uniform(-3, 3, (n, 2)).astype(F)
    whole = rng.random(n) < 0.15
    motion[whole, :2] = rng.integers(-2, 3, (int(whole.sum()), 2)).astype(F)
    gone = rng.random(n) < 0.10
    motion[gone, :2] = np.inf
    motion[:, 2] = z0
    motion[gone & (rng.random(n) < 0.5), 2] = -1.0
    depth = (z0 * (1.0 + 0.2 * rng.uniform(-1, 1, n))).astype(F)
    bad = rng.random(n) < 0.10
    kind = rng.integers(0, 4, n)
    depth[bad & (kind == 0)] = 0.0
    depth[bad & (kind == 1)] = -1.0
    depth[bad & (kind == 2)] = np.inf
    depth[bad & (kind == 3)] = np.nan
    motion[:, 3] = depth
    xx = np.arange(n) % w
    band = np.minimum(3 * xx // max(w, 1), 2)
    noise = np.array([0.3, 1.5, 10.0])[band] * DEPTH_TOL
    motion_prev = rng.uniform(-3, 3, (n, 4)).astype(F)  # only .w is read
    motion_prev[:, 3] = (z0 * (1.0 + noise * rng.uniform(-1, 1, n))).astype(F)
    odd = rng.random(n) < 0.05
    motion_prev[odd, 3] = np.where(rng.random(int(odd.sum())) < 0.5, np.inf, np.nan)
    out = dict(w=w, h=h, W=W, H=H, color_cur=rng.random((n, 4)).astype(F), motion_cur=motion, motion_prev=motion_prev,
               color_prev=rng.random((N, 4)).astype(F), hist_prev=rng.integers(1, 40, N).astype(F))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _SYN[key] = out
    return out
