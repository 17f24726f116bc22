"""A float32 numpy restatement of the deferred reflection passes (rt_device.hpp: reflection_mirror, reflection_base,
reflection_direction, reflection_origin, reflection_miss_color, reflection_light_add, reflection_hit_color,
reflection_reduce, reflection_composite_pixel; include/rt_api.h: rt_dispatch_reflection, rt_host_reflection_rays,
rt_host_reflection_radiance, rt_reflection_composite, rt_host_reflection_composite).

Every operation is one rounded float32 (numpy rounds each array operation; nothing is fused), in the header's order, so
the host services must equal the three functions here bit for bit. The hash, the sphere point, the normal's validity
and the facing normal are tests/ao_reference.py's, the light test, the camera rays and the RGBA8 packing
tests/shadow_reference.py's (the reflection pass calls those passes' functions).
"""
import numpy as np

import ao_reference as ao
import shadow_reference as sh

F = np.float32
U = np.uint32


def reflect_dir(i, n):
    """HLSL reflect(i, n), evaluated as i - (2 n) * dot(i, n)."""
    t = ao.dot(i, n).astype(F)
    return (i - (F(2.0) * n) * t[..., None]).astype(F)


def mirror(D, nn):
    return ao.normalize(ao.normalize(reflect_dir(ao.normalize(D).astype(F), nn)).astype(F)).astype(F)


def reflection_base(px, py, seed):
    pass_seed = np.array([seed], U) ^ ao.ao_hash(np.array([0x100], U))  # arrays: uint32 that wraps without a warning
    return ao.ao_hash(np.asarray(px, U) + ao.ao_hash(np.asarray(py, U) + ao.ao_hash(pass_seed)))


def direction(m, nf, roughness, base, k):
    """-> d_k (n, 3), fell_back (n,): the samples that the horizon rule replaced by the mirror direction."""
    if F(roughness) == 0:
        return m, np.zeros(m.shape[0], bool)
    v = (m + ao.ao_sphere(base, k) * F(roughness)).astype(F)
    small = ao.dot(v, v) < F(1e-4)
    d = np.where(small[:, None], m, ao.normalize(v)).astype(F)
    above = ao.dot(d, nf) > 0
    return np.where(above[:, None], d, m).astype(F), ~above


def host_reflection_rays(cam_rays, t, normal, px, py, samples=1, roughness=0.0, tmax=1000.0, shadow_tmin=0.01, seed=0,
                         want_fallback=False):
    """rt.host_reflection_rays restated: -> rays (n, samples, 8) float32, valid (n,) uint8 (and, asked for, the
    (n, samples) mask of the samples below the horizon)."""
    cam = np.asarray(cam_rays, F).reshape(-1, 8)
    t = np.asarray(t, F).ravel()
    n3 = np.asarray(normal, F).reshape(-1, 4)[:, :3]
    O, D = cam[:, 0:3], cam[:, 4:7]
    valid = ao.normal_valid(n3)
    rays = np.zeros((cam.shape[0], samples, 8), F)
    fell = np.zeros((cam.shape[0], samples), bool)
    with np.errstate(all="ignore"):
        nn = ao.normalize(n3).astype(F)
        m = mirror(D, nn)
        nf = ao.facing_normal(nn, D)
        P = (O + D * t[:, None]).astype(F)
        base = reflection_base(px, py, seed)
        for k in range(samples):
            d, fell[:, k] = direction(m, nf, roughness, base, k)
            rays[:, k, 0:3] = (P + d * F(0.001)).astype(F)
            rays[:, k, 3] = F(0.001)
            rays[:, k, 4:7] = d
            rays[:, k, 7] = F(tmax)
    rays[~valid] = 0
    fell[~valid] = False
    return (rays, valid.astype(np.uint8), fell) if want_fallback else (rays, valid.astype(np.uint8))


def host_reflection_radiance(rays, hits, hit_normal, hit_group, occluded, valid, py, height, lights, tmax=1000.0):
    """rt.host_reflection_radiance restated: -> radiance (n, 4) float32, lit (n, S, nlights) uint8."""
    rays = np.asarray(rays, F)
    n, S = rays.shape[0], rays.shape[1]
    hits = np.ascontiguousarray(hits).view(U).reshape(n, S, 4)
    hn = np.asarray(hit_normal, F).reshape(n, S, 4)
    hg = np.asarray(hit_group, U).reshape(n, S)
    lps = sh.positions(lights)
    occ = np.asarray(occluded).reshape(n, S, len(lps)) != 0
    valid = np.asarray(valid).ravel() != 0
    ramp = np.asarray(py, U).astype(F) / F(height)
    sky = np.stack([np.zeros(n, F), np.full(n, F(0.2)), F(0.7) - F(0.3) * ramp], axis=1).astype(F)
    sumL, sumt = np.zeros((n, 3), F), np.zeros(n, F)
    lit = np.zeros((n, S, len(lps)), np.uint8)
    with np.errstate(all="ignore"):
        for k in range(S):
            found = hits[:, k, 3] != 0
            t2 = np.ascontiguousarray(hits[:, k, 0]).view(F)
            ro, d = rays[:, k, 0:3], rays[:, k, 4:7]
            ns = sh.shading_normal(hn[:, k], hg[:, k])
            P2 = (ro + d * t2[:, None]).astype(F)
            c = np.zeros(n, F)
            for l, lp in enumerate(lps):
                _, nl, is_lit = sh.lit_rule(ns, lp, P2)
                is_lit = is_lit & found & valid
                lit[:, k, l] = is_lit
                term = (c + nl * np.where(occ[:, k, l], F(0.3), F(1.0))).astype(F)
                c = np.where(is_lit, term, c).astype(F)
            c = (c / F(len(lps))).astype(F)
            L = np.where(found[:, None], np.repeat(c[:, None], 3, axis=1), sky).astype(F)
            sumL = (sumL + L).astype(F)
            sumt = (sumt + np.where(found, t2, F(tmax))).astype(F)
        out = np.concatenate([sumL / F(S), (sumt / F(S))[:, None]], axis=1).astype(F)
    out[~valid] = 0
    return out, lit


def host_reflection_composite(width, height, cb, color_in, radiance, hits, normal, strength=1.0, f0=0.04):
    """rt.host_reflection_composite restated: -> color (n, 4) float32, rgba8 (n, 4) uint8."""
    n = width * height
    base = np.asarray(color_in, F).reshape(n, 4)
    refl = np.asarray(radiance, F).reshape(n, 4)
    hits = np.ascontiguousarray(hits).view(U).reshape(n, 4)
    n3 = np.asarray(normal, F).reshape(n, 4)[:, :3]
    _, D = sh.pixel_rays(cb, width, height)
    on = (hits[:, 3] != 0) & ao.normal_valid(n3)
    with np.errstate(all="ignore"):
        nf = ao.facing_normal(ao.normalize(n3).astype(F), D)
        x = np.minimum(np.maximum(F(1.0) - np.maximum(ao.dot(nf, -D), F(0.0)), F(0.0)), F(1.0)).astype(F)
        x2 = x * x
        x5 = (x2 * x2) * x
        fres = F(f0) + (F(1.0) - F(f0)) * x5
        k = (F(strength) * fres).astype(F)
        mixed = (base[:, :3] + k[:, None] * (refl[:, :3] - base[:, :3])).astype(F)
    color = base.copy()
    color[on, :3] = mixed[on]
    color[on, 3] = F(1.0)
    rgba8 = np.full((n, 4), 255, np.uint8)
    rgba8[:, :3] = sh.unorm8(color[:, :3])
    return color, rgba8
