"""The radiance filter (rt_radiance_accumulate, rt_radiance_atrous; include/rt_api.h) restated in numpy float32, from
the header's text alone, in tests/denoise_reference.py's style: every operation is one float32 numpy operation in the
header's order, so the host twins must equal it bit for bit. Also the synthetic radiance planes the CPU and GPU tests
share (the guide, motion and normal planes are denoise_reference.synthetic's, imported, not edited).

Planes are flat, row-major: entry y * W + x. Each pass also returns the per-pixel branch classes the tests count."""
import numpy as np

from denoise_reference import BIG, F, H5, SIZES, _dot, _maxf, _minf, guide, synthetic  # noqa: F401  (re-exported)

DEPTH_TOL, NORMAL_COS, SIGMA_L = 0.02, 0.9, 4.0


def lum(c):
    return ((F(0.2126) * c[:, 0] + F(0.7152) * c[:, 1]) + F(0.0722) * c[:, 2]).astype(F)


def _wn(g, q, ncos, nden):
    return _minf(F(1.0), _maxf(F(0.0), (_dot(g[:, 0], g[:, 1], g[:, 2], q[:, 0], q[:, 1], q[:, 2]) - ncos) / nden))


def accumulate(W, H, rad_cur, motion, guide_cur, rad_prev=None, moments_prev=None, guide_prev=None, max_history=32,
               depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS):
    """-> rad_out (n, 4), moments_out (n, 4), cls: a dict of (n,) bool planes: no_surface, disocclusion (a surface
    without a usable history: the first frame too), blended, spatial (the spatial variance estimate was taken)."""
    n = W * H
    c = np.asarray(rad_cur, F).reshape(n, 4)
    m = np.asarray(motion, F).reshape(n, 4)
    g = np.asarray(guide_cur, F).reshape(n, 4)
    yy, xx = np.divmod(np.arange(n), W)
    surface = g[:, 3] != 0
    tol, ncos = F(depth_tol), F(normal_cos)
    l = lum(c)
    sw, s1, s2, sh = (np.zeros(n, F) for _ in range(4))
    sc = np.zeros((n, 4), F)
    with np.errstate(all="ignore"):
        if rad_prev is not None:
            rp = np.asarray(rad_prev, F).reshape(n, 4)
            mp = np.asarray(moments_prev, F).reshape(n, 4)
            q = np.asarray(guide_prev, F).reshape(n, 4)
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
                inside = seek & (w != 0) & (px >= 0) & (py >= 0) & (px < W) & (py < H)
                t = np.where(inside, py * W + px, 0)
                qt = q[t]
                ok = inside & (qt[:, 3] != 0) & ~(np.abs(qt[:, 3] - m[:, 2]) > lim)
                ok &= ~(_dot(g[:, 0], g[:, 1], g[:, 2], qt[:, 0], qt[:, 1], qt[:, 2]) < ncos)
                sw = np.where(ok, sw + w, sw).astype(F)
                for ch in range(4):
                    sc[:, ch] = np.where(ok, sc[:, ch] + w * rp[t, ch], sc[:, ch])
                s1 = np.where(ok, s1 + w * mp[t, 0], s1).astype(F)
                s2 = np.where(ok, s2 + w * mp[t, 1], s2).astype(F)
                sh = np.where(ok, sh + w * mp[t, 2], sh).astype(F)
        blend = surface & (sw >= F(0.01))
        cnt = _minf(sh / sw + F(1.0), F(max_history))
        a = F(1.0) / cnt
        mix = blend & (cnt != F(1.0))

        def blended(s, cur):
            p = (s / sw).astype(F)
            return np.where(mix, p + a * (cur - p), cur).astype(F)

        rad = np.stack([blended(sc[:, ch], c[:, ch]) for ch in range(4)], axis=1)
        m1, m2 = blended(s1, l), blended(s2, (l * l).astype(F))
        hist = np.where(blend, cnt, F(1.0)).astype(F)
        var_t = _maxf(F(0.0), m2 - m1 * m1)
        # the spatial estimate
        zden, nden = tol * g[:, 3], F(1.0) - ncos
        tw, t1, t2 = (np.zeros(n, F) for _ in range(3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                px, py = xx + dx, yy + dy
                inside = (px >= 0) & (py >= 0) & (px < W) & (py < H)
                t = np.where(inside, py * W + px, 0)
                q = g[t]
                if dx == 0 and dy == 0:
                    ok, w = inside, np.ones(n, F)
                else:
                    ok = inside & (q[:, 3] != 0)
                    wz = _maxf(F(0.0), F(1.0) - np.abs(q[:, 3] - g[:, 3]) / zden)
                    w = (wz * _wn(g, q, ncos, nden)).astype(F)
                lt = lum(c[t])
                tw = np.where(ok, tw + w, tw).astype(F)
                t1 = np.where(ok, t1 + w * lt, t1).astype(F)
                t2 = np.where(ok, t2 + w * (lt * lt), t2).astype(F)
        M1, M2 = t1 / tw, t2 / tw
        var_s = (_maxf(F(0.0), M2 - M1 * M1) * (F(4.0) / hist)).astype(F)
        spatial = surface & ~(hist >= F(4.0))
        var = np.where(spatial, var_s, var_t).astype(F)
    mom = np.stack([m1, m2, hist, var], axis=1).astype(F)
    mom[~surface] = 0.0
    rad[~surface] = c[~surface]
    cls = dict(no_surface=~surface, disocclusion=surface & ~blend, blended=blend, spatial=spatial)
    return rad, mom, cls


def atrous_iteration(W, H, s, src, var, g, depth_tol, normal_cos, sigma_l):
    """-> colour (n, 4), variance (n,), wl_zero, wl_partial: (n,) counts of a pixel's taken non-centre taps whose
    luminance weight was 0 and strictly between 0 and 1."""
    n = W * H
    yy, xx = np.divmod(np.arange(n), W)
    surface = g[:, 3] != 0
    tol, ncos, sig = F(depth_tol), F(normal_cos), F(sigma_l)
    with np.errstate(all="ignore"):
        pw, pv = np.zeros(n, F), np.zeros(n, F)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                w = F((0.5 if dy == 0 else 0.25) * (0.5 if dx == 0 else 0.25))
                px, py = xx + dx * s, yy + dy * s
                inside = (px >= 0) & (py >= 0) & (px < W) & (py < H)
                t = np.where(inside, py * W + px, 0)
                pw = np.where(inside, pw + w, pw).astype(F)
                pv = np.where(inside, pv + w * var[t], pv).astype(F)
        lden = (sig * np.sqrt((pv / pw).astype(F)) + F(1e-4)).astype(F)
        lc = lum(src)
        zden = (tol * g[:, 3]) * F(s)
        nden = F(1.0) - ncos
        sw, sv = np.zeros(n, F), np.zeros(n, F)
        sc = np.zeros((n, 4), F)
        wl_zero, wl_partial = np.zeros(n, int), np.zeros(n, int)
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
                    wl = _maxf(F(0.0), F(1.0) - np.abs(lum(src[t]) - lc) / lden)
                    e = ((wz * _wn(g, q, ncos, nden)) * wl).astype(F)
                    w = (k * (e * e)).astype(F)
                    wl_zero += ok & surface & (wl == 0)
                    wl_partial += ok & surface & (wl > 0) & (wl < 1)
                sw = np.where(ok, sw + w, sw).astype(F)
                for ch in range(4):
                    sc[:, ch] = np.where(ok, sc[:, ch] + w * src[t, ch], sc[:, ch])
                sv = np.where(ok, sv + (w * w) * var[t], sv).astype(F)
        col = (sc / sw[:, None]).astype(F)
        vo = (sv / (sw * sw)).astype(F)
    col[~surface] = src[~surface]
    vo = np.where(surface, vo, var).astype(F)
    return col, vo, wl_zero, wl_partial


def atrous(W, H, rad_in, moments, guide_plane, iterations=3, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS,
           sigma_l=SIGMA_L):
    """-> rad_out (n, 4), var_out (n,), cls: wl_zero and wl_partial, (n,) counts summed over the iterations."""
    n = W * H
    g = np.asarray(guide_plane, F).reshape(n, 4)
    col = np.asarray(rad_in, F).reshape(n, 4)
    var = np.asarray(moments, F).reshape(n, 4)[:, 3]
    z, p = np.zeros(n, int), np.zeros(n, int)
    for k in range(iterations):
        col, var, wz, wp = atrous_iteration(W, H, 1 << k, col, var, g, depth_tol, normal_cos, sigma_l)
        z, p = z + wz, p + wp
    return col, var, dict(wl_zero=z, wl_partial=p)


_SYN = {}


def synthetic_radiance(W, H, seed=0):
    """Radiance planes to go with denoise_reference.synthetic(W, H, seed) (shared, read-only). rad_cur: a colour that
    is smooth within the three bands, with a noise whose amplitude grows with x inside a band (so the luminance weight
    is 1, partial and 0 somewhere) and a tenth of the pixels fireflies; .w a distance in 0.5 .. 20. rad_prev: another
    draw. moments_prev: (m1, m2, hist, var) with hist 0 .. 39, a third of it below 4, so that a blended pixel takes the
    spatial estimate as well as the temporal one."""
    key = (W, H, seed)
    if key in _SYN:
        return _SYN[key]
    rng = np.random.default_rng(2000 * seed + 11 * W + H)
    n = W * H
    yy, xx = np.divmod(np.arange(n), W)
    u = (3 * xx % max(W, 1)) / max(W, 1)  # 0 .. 1 across a band

    def plane():
        base = np.stack([0.2 + 0.5 * u, 0.6 - 0.3 * u, 0.3 + 0.1 * yy / max(H, 1)], axis=1)
        noise = (0.002 + 0.4 * u ** 2)[:, None] * rng.uniform(-1, 1, (n, 3))
        rgb = np.abs(base + noise)
        fire = rng.random(n) < 0.10
        rgb[fire] *= rng.uniform(3, 30, (int(fire.sum()), 1))
        return np.concatenate([rgb, rng.uniform(0.5, 20.0, (n, 1))], axis=1).astype(F)

    cur, prev = plane(), plane()
    lp = lum(prev).astype(np.float64)
    hist = rng.integers(0, 40, n)
    short = rng.random(n) < 0.33
    hist[short] = rng.integers(0, 4, int(short.sum()))
    mom = np.stack([lp, lp * lp + rng.uniform(0, 0.05, n), hist, rng.uniform(0, 0.05, n)], axis=1).astype(F)
    out = dict(rad_cur=cur, rad_prev=prev, moments_prev=mom)
    for v in out.values():
        v.setflags(write=False)
    _SYN[key] = out
    return out
