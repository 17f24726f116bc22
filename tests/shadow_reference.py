"""A float32 numpy restatement of the soft-shadow passes (rt_device.hpp: pixel_ray, shading_normal, shadow_lit,
shadow_base, shadow_direction, resolve_pixel; include/rt_api.h: rt_dispatch_shadow, rt_host_shadow_rays,
rt_shade_resolve, rt_host_shade_resolve).

Every operation is one rounded float32 (numpy rounds each array operation; nothing is fused), in the header's order,
so the host services must equal host_shadow_rays() and host_shade_resolve() here bit for bit. The hash and the sphere
point are tests/ao_reference.py's (the AO pass's, which the shadow pass calls).
"""
import numpy as np

import ao_reference as ao

F = np.float32
U = np.uint32
PLANE = 2  # RT_HITGROUP_PLANE
TMAX = F(100000.0)


def positions(lights):
    """(nlights, 3) float32 from set_shading's (colour, position, intensity) triples."""
    return np.array([[F(v) for v in pos] for (_, pos, _) in lights], F).reshape(-1, 3)


def shading_normal(normal, hit_group):
    n3 = np.asarray(normal, F).reshape(-1, 4)[:, :3]
    g = np.asarray(hit_group, U).ravel()
    return np.where((g == PLANE)[:, None], n3, -n3).astype(F)


def lit_rule(ns, lp, P):
    """-> L (n, 3), nl (n,), lit (n,): the frame kernels' expressions; a NaN nl is not lit."""
    with np.errstate(all="ignore"):
        L = ao.normalize((lp[None, :] - P).astype(F)).astype(F)
        nl = ao.dot(ns, L).astype(F)
        return L, nl, nl > 0


def shadow_base(px, py, seed, l):
    light_seed = np.array([seed], U) ^ ao.ao_hash(np.array([l + 1], U))  # arrays: uint32 that wraps without a warning
    return ao.ao_hash(np.asarray(px, U) + ao.ao_hash(np.asarray(py, U) + ao.ao_hash(light_seed)))


def direction(lp, radius, base, k, P):
    target = np.broadcast_to(lp[None, :], P.shape).astype(F)
    if F(radius) != 0:
        target = (target + ao.ao_sphere(base, k) * F(radius)).astype(F)
    with np.errstate(all="ignore"):
        return ao.normalize(ao.normalize((target - P).astype(F)).astype(F)).astype(F)


def host_shadow_rays(cam_rays, t, normal, hit_group, px, py, lights, samples=1, light_radius=0.0, tmin=0.01, seed=0):
    """rt.host_shadow_rays restated: -> rays (n, nlights, samples, 8) float32, lit (n, nlights) uint8."""
    cam = np.asarray(cam_rays, F).reshape(-1, 8)
    t = np.asarray(t, F).ravel()
    lps = positions(lights)
    n = cam.shape[0]
    O, D = cam[:, 0:3], cam[:, 4:7]
    ns = shading_normal(normal, hit_group)
    rays = np.zeros((n, lps.shape[0], samples, 8), F)
    lit = np.zeros((n, lps.shape[0]), np.uint8)
    with np.errstate(all="ignore"):
        P = (O + D * t[:, None]).astype(F)
        for l, lp in enumerate(lps):
            _, _, is_lit = lit_rule(ns, lp, P)
            lit[:, l] = is_lit
            base = shadow_base(px, py, seed, l)
            for k in range(samples):
                rays[:, l, k, 0:3] = P
                rays[:, l, k, 3] = F(tmin)
                rays[:, l, k, 4:7] = direction(lp, light_radius, base, k, P)
                rays[:, l, k, 7] = TMAX
            rays[~is_lit, l] = 0
    return rays, lit


def hlsl_mul4(mem, v):
    """HLSL mul(M, v), M column-major in XMMATRIX memory: r_i = ((m[i] v0 + m[4+i] v1) + m[8+i] v2) + m[12+i] v3."""
    mem = np.asarray(mem, F)
    return np.stack([((mem[i] * v[0] + mem[4 + i] * v[1]) + mem[8 + i] * v[2]) + mem[12 + i] * v[3] for i in range(4)],
                    axis=-1).astype(F)


def pixel_rays(cb, width, height):
    """The camera rays of a whole frame through the pixel centres: O (3,), D (n, 3), row-major."""
    cb = np.asarray(cb, F).ravel()
    py, px = np.divmod(np.arange(width * height, dtype=U), U(width))
    dx = ((px.astype(F) + F(0.5)) / F(width)) * F(2.0) - F(1.0)
    dy = ((py.astype(F) + F(0.5)) / F(height)) * F(2.0) - F(1.0)
    one = np.ones_like(dx)
    dc = hlsl_mul4(cb[48:64], (dx, -dy, one, one))
    dw = hlsl_mul4(cb[32:48], (dc[:, 0], dc[:, 1], dc[:, 2], np.zeros_like(dx)))
    origin = hlsl_mul4(cb[32:48], (F(0.0), F(0.0), F(0.0), F(1.0)))
    return origin[:3].astype(F), ao.normalize(dw[:, :3].astype(F)).astype(F)


def unorm8(c):
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        v = (c * F(255.0) + F(0.5)).astype(F)
        out = np.where(c >= 1, 255, np.where(c > 0, v, 0).astype(np.uint32))
    return np.where(c > 0, out, 0).astype(np.uint8)


def host_shade_resolve(width, height, cb, lights, hits, normal, obj, vis=None, ao_plane=None):
    """rt.host_shade_resolve restated: -> color (n, 4) float32, rgba8 (n, 4) uint8."""
    n = width * height
    hits = np.ascontiguousarray(hits).view(U).reshape(n, 4)
    obj = np.ascontiguousarray(obj).view(U).reshape(n, 2)
    lps = positions(lights)
    O, D = pixel_rays(cb, width, height)
    t = np.ascontiguousarray(hits[:, 0]).view(F)
    a = np.ones(n, F) if ao_plane is None else np.asarray(ao_plane, F).ravel()
    with np.errstate(all="ignore"):
        P = (O[None, :] + D * t[:, None]).astype(F)
        ns = shading_normal(normal, obj[:, 1])
        c = np.zeros(n, F)
        for l, lp in enumerate(lps):
            _, nl, is_lit = lit_rule(ns, lp, P)
            v = np.ones(n, F) if vis is None else np.asarray(vis, F).reshape(len(lps), n)[l]
            term = (c + nl * ((F(0.3) * a) + (F(0.7) * v))).astype(F)
            c = np.where(is_lit, term, c).astype(F)
        c = (c / F(len(lps))).astype(F)
    y = (np.arange(n, dtype=U) // U(width)).astype(F)
    ramp = y / F(height)
    miss = hits[:, 3] == 0
    color = np.ones((n, 4), F)
    color[:, 0] = np.where(miss, F(0.0), c)
    color[:, 1] = np.where(miss, F(0.2), c)
    color[:, 2] = np.where(miss, F(0.7) - F(0.3) * ramp, c)
    rgba8 = np.full((n, 4), 255, np.uint8)
    rgba8[:, :3] = unorm8(color[:, :3])
    return color, rgba8
