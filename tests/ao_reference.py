"""A float32 numpy restatement of the ambient-occlusion sample generator (rt_device.hpp: ao_hash, det_sincos_2pi,
ao_sphere, ao_normal_valid, ao_facing_normal, ao_direction; include/rt_api.h: rt_dispatch_ao, rt_host_ao_rays).

Every operation is one rounded float32 (numpy rounds each array operation; nothing is fused), in the header's order,
so rt_host_ao_rays must equal host_ao_rays() here bit for bit. Integers are uint32 arrays, which wrap.
"""
import numpy as np

F = np.float32
U = np.uint32

# the polynomials of det_sincos_2pi, as pinned in rt_device.hpp: the Taylor coefficients of sin (degree 9) and cos
# (degree 8), each rounded to float32
TWO_PI = F(6.2831853)
SIN_C = (F(-1.66666672e-01), F(8.33333377e-03), F(-1.98412701e-04), F(2.75573188e-06))
COS_C = (F(-5.0e-01), F(4.16666679e-02), F(-1.38888892e-03), F(2.48015876e-05))
# max |error| of det_sincos_2pi against float64 cos / sin of 2 pi u over all 2^24 inputs u = k 2^-24, measured on the
# CPU (test_ao_host.py asserts this exact value; DESIGN §3.9 records it)
SINCOS_MAX_ERR = 9.304034753743196e-08


def ao_hash(v):
    v = np.asarray(v, U)
    v = v * U(747796405) + U(2891336453)
    w = ((v >> ((v >> U(28)) + U(4))) ^ v) * U(277803737)
    return (w >> U(22)) ^ w


def ao_base(px, py, seed):
    return ao_hash(np.asarray(px, U) + ao_hash(np.asarray(py, U) + ao_hash(U(seed))))


def det_sincos_2pi(u):
    """(cos, sin) of 2 pi u for float32 u in [0, 1)."""
    u = np.asarray(u, F)
    q = np.floor(F(4.0) * u + F(0.5))
    f = u - F(0.25) * q
    x = TWO_PI * f
    x2 = x * x
    ps = SIN_C[3]
    ps = ps * x2 + SIN_C[2]
    ps = ps * x2 + SIN_C[1]
    ps = ps * x2 + SIN_C[0]
    ps = ps * x2 + F(1.0)
    s = x * ps
    pc = COS_C[3]
    pc = pc * x2 + COS_C[2]
    pc = pc * x2 + COS_C[1]
    pc = pc * x2 + COS_C[0]
    c = pc * x2 + F(1.0)
    k = q.astype(np.int32).astype(U) & U(3)
    cos = np.where(k == 0, c, np.where(k == 1, -s, np.where(k == 2, -c, s)))
    sin = np.where(k == 0, s, np.where(k == 1, c, np.where(k == 2, -s, -c)))
    return cos.astype(F), sin.astype(F)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(a):
    """rt_device.hpp normalize: v * (1 / sqrt(dot(v, v)))."""
    inv = F(1.0) / np.sqrt(dot(a, a))
    return a * inv[..., None]


def ao_sphere(base, k):
    """Sample k of the pixels whose hash base is `base`: a point uniform on the unit sphere, (n, 3)."""
    base = np.asarray(base, U)
    a = ao_hash(base + U(2) * U(k))
    b = ao_hash(base + U(2) * U(k) + U(1))
    u1 = (a >> U(8)).astype(F) * F(2.0 ** -24)
    u2 = (b >> U(8)).astype(F) * F(2.0 ** -24)
    z = F(1.0) - F(2.0) * u1
    r = np.sqrt(np.maximum(F(0.0), F(1.0) - z * z))
    c, s = det_sincos_2pi(u2)
    return np.stack([r * c, r * s, z], axis=-1).astype(F)


def normal_valid(n):
    with np.errstate(all="ignore"):
        d = dot(n, n)
        return np.isfinite(n).all(axis=-1) & np.isfinite(d) & (d > 0)


def facing_normal(n, D):
    nn = normalize(n)
    away = dot(nn, D) > 0
    return np.where(away[..., None], -nn, nn).astype(F)


def direction(nf, sph):
    v = nf + sph
    small = dot(v, v) < F(1e-4)
    with np.errstate(all="ignore"):
        return np.where(small[..., None], nf, normalize(v)).astype(F)


def host_ao_rays(cam_rays, t, normal, px, py, samples, radius, tmin=0.01, seed=0):
    """rt.host_ao_rays restated: -> rays (n, samples, 8) float32, valid (n,) uint8."""
    cam = np.asarray(cam_rays, F).reshape(-1, 8)
    t = np.asarray(t, F).ravel()
    n3 = np.asarray(normal, F).reshape(-1, 4)[:, :3]
    O, D = cam[:, 0:3], cam[:, 4:7]
    valid = normal_valid(n3)
    with np.errstate(all="ignore"):
        nf = facing_normal(n3, D)
        P = (O + D * t[:, None]).astype(F)
        base = ao_base(px, py, seed)
        rays = np.zeros((cam.shape[0], samples, 8), F)
        for k in range(samples):
            d = direction(nf, ao_sphere(base, k))
            rays[:, k, 0:3] = P
            rays[:, k, 3] = F(tmin)
            rays[:, k, 4:7] = d
            rays[:, k, 7] = F(radius)
    rays[~valid] = 0
    return rays, valid.astype(np.uint8)
