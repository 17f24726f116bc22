"""The PBR resolve restated in float64 numpy (rt_shade_resolve_pbr, rt_host_shade_resolve_pbr; include/rt_api.h), and
what the two test files of the pass share: the materials, the G-buffer planes of a scene from the CPU oracle, the
visibility planes of hard shadows, and the rule that gives a pixel its material.

resolve_f64 is transcribed from the HLSL (Hit.hlsl:83-174 and :207-241, Miss.hlsl:8), not from the library: quotients
and powers as numpy evaluates them, in float64, over the float32 planes. It shares no text with rt_device.hpp, so it
agrees with the library to a tolerance (1e-4 L-inf, the bound tests/test_oracle.py holds the oracle's REF frames to
against oracle/np_reference.py), not to the bit. The exact expectations of the tests come from unchanged RT_SHADE_REF
frames instead.
"""
import numpy as np

import realtimeraytracing_gradproject_amd as rt
from realtimeraytracing_gradproject_amd import scenes

import oracle
from oracle import np_reference

PI = 3.14159265359  # Common.hlsl:1
MODEL, PLANE = rt.RT_HITGROUP_MODEL, rt.RT_HITGROUP_PLANE
MISS = 0xFFFFFFFF

# K = 4 distinct materials with reflectivity 0: albedo rgb, roughness 0.2 .. 0.9, metallic 0 .. 1
MATERIALS = [(1.0, 1.0, 1.0, 0.5, 0.5, 0.0), (0.9, 0.15, 0.1, 0.2, 0.0, 0.0), (0.1, 0.7, 0.25, 0.9, 1.0, 0.0),
             (0.2, 0.3, 0.95, 0.35, 0.75, 0.0)]
# instances 0, 1, 3, 4, 5 of the reference scene (2 coincides with 1 and never wins, 6 is the plane) -> four entries
INSTANCE_MATERIAL = np.array([1, 2, 2, 3, 0, 1, 3], np.uint32)


def reflo(w, h):
    """REFLO with reflectivity 0: the reference scene seen from outside."""
    s = scenes.config("REFLO").with_size(w, h)
    s.material = s.material[:5] + (0.0,)
    s.mode = rt.RT_SHADE_REF
    return s


def material_index(obj, instance_material, nmaterials):
    """rt_shade_resolve_pbr's rule: m = map ? (inst < len(map) ? map[inst] : 0) : 0, then m < nmaterials ? m : 0."""
    inst = obj[:, 0].astype(np.int64)
    m = np.zeros(inst.size, np.int64)
    if instance_material is not None:
        im = np.asarray(instance_material, np.int64)
        inside = inst < im.size
        m[inside] = im[inst[inside]]
    m[m >= nmaterials] = 0
    return m


def pixels(w, h):
    py, px = np.divmod(np.arange(w * h, dtype=np.uint32), np.uint32(w))
    return px, py


def oracle_gbuffer(spec):
    """hits (n, 4) uint32, normal (n, 4) float32, object (n, 2) uint32 of the full frame, as rt_dispatch_gbuffer writes
    them: the CPU oracle's closest hits of RayGen's own rays, rt.host_shading_normals per instance, the scene list."""
    px, py = pixels(spec.width, spec.height)
    rays = oracle.camera_rays(spec.camera_buffer(), spec.width, spec.height, px, py)
    hits, uv, _ = oracle.Scene(spec).trace_rays(rays)
    hit = hits[:, 3] == 1
    group = np.array([hg for (_, _, _, hg) in spec.instances], np.uint32)
    obj = np.full((hits.shape[0], 2), MISS, np.uint32)
    obj[hit, 0] = hits[hit, 1]
    obj[hit, 1] = group[hits[hit, 1]]
    normal = np.zeros((hits.shape[0], 4), np.float32)
    for k, (m, x, _, hg) in enumerate(spec.instances):
        sel = hit & (hits[:, 1] == k)
        if sel.any():
            v, i = spec.meshes[m]
            normal[sel] = rt.host_shading_normals(v, i, hits[sel, 2], uv[sel], hg, x)
    return hits, normal, obj


def hard_shadow_planes(spec, planes):
    """(nlights, n) float32: rt_dispatch_shadow's planes at light_radius 0, one sample, tmin 0.01, from
    rt.host_shadow_rays and the CPU oracle's any-hit search: 1 on a miss, 0 where the pixel does not face the light or
    its ray is occluded, else 1."""
    hits, normal, obj = planes
    px, py = pixels(spec.width, spec.height)
    cam = oracle.camera_rays(spec.camera_buffer(), spec.width, spec.height, px, py)
    rays, lit = rt.host_shadow_rays(cam, hits[:, 0].view(np.float32), normal, obj[:, 1], px, py, spec.lights, 1, 0.0,
                                    0.01, 0)
    hit = hits[:, 3] == 1
    lit = (lit == 1) & hit[:, None]
    occ = np.zeros(lit.shape, bool)
    if lit.any():
        h, _, _ = oracle.Scene(spec).trace_rays(rays[lit].reshape(-1, 8), any_hit=True)
        occ[lit] = h[:, 3] == 1
    vis = np.where(hit[:, None], (lit & ~occ).astype(np.float32), np.float32(1.0))
    return np.ascontiguousarray(vis.T, np.float32)


def classes(planes):
    """-> miss, plane, model: boolean pixel classes from the hits and object planes."""
    hits, _, obj = planes
    hit = hits[:, 3] != 0
    return ~hit, hit & (obj[:, 1] == PLANE), hit & (obj[:, 1] != PLANE)


def assert_input_conditions(planes, vis0=None):
    """What the checks need of a REFLO G-buffer, so that a later change of the scene cannot hollow them out."""
    miss, plane, model = classes(planes)
    counts = np.bincount(planes[2][model, 0].astype(np.int64), minlength=8)
    assert (counts >= 8).sum() >= 5, f"fewer than five model instances with 8 pixels: {counts}"
    assert miss.sum() >= 100, f"{miss.sum()} miss pixels"
    if vis0 is not None:
        dark = plane & (vis0 == 0)
        assert dark.sum() >= 40 and (plane & (vis0 == 1)).sum() >= 40, f"{dark.sum()} shadowed plane pixels"


def _norm(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def normal_valid(n):
    """rt_dispatch_reflection's rule on float32 normals: every component finite, dot(n, n) finite and > 0."""
    n = np.asarray(n, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]).astype(np.float32)
    return np.isfinite(n[:, :3]).all(axis=1) & np.isfinite(d) & (d > 0)


def resolve_f64(width, height, cb, lights, hits, normal, obj, materials, instance_material=None, vis=None, ao=None,
                refl=None):
    """-> (n, 3) float64 colours. The HLSL's formulas with s_l = 0.3 a + 0.7 v_l on each light's two terms."""
    n = width * height
    px, py = pixels(width, height)
    O, D = np_reference.camera_rays(np.asarray(cb), width, height, px.astype(float), py.astype(float))
    t = hits[:, 0].view(np.float32).astype(np.float64)
    P = O + D * t[:, None]
    N = normal[:, :3].astype(np.float64)
    a = np.ones(n) if ao is None else np.asarray(ao, np.float64).ravel()
    nl = len(lights)
    v = np.ones((nl, n)) if vis is None else np.asarray(vis, np.float64).reshape(nl, n)
    s = 0.3 * a[None, :] + 0.7 * v
    miss, plane, model = classes((hits, normal, obj))
    out = np.zeros((n, 3))
    out[miss] = np.stack([np.zeros(miss.sum()), np.full(miss.sum(), 0.2), 0.7 - 0.3 * (py[miss] / height)], -1)
    # PlaneClosestHit: light 0 only, no material
    ld = _norm(np.asarray(lights[0][1], float) - P[plane])
    out[plane] = (np.maximum(0.0, np.sum(N[plane] * ld, -1)) * s[0, plane])[:, None]
    # ClosestHit
    mats = np.asarray(materials, np.float64)
    m = material_index(obj, instance_material, len(materials))[model]
    albedo, rough, metal, reflectivity = mats[m, :3], mats[m, 3:4], mats[m, 4:5], mats[m, 5]
    Pm, nm = P[model], N[model]
    Nn = -_norm(nm)
    V = _norm(O[model] - Pm)
    cd = np.zeros_like(Pm)
    L0 = np.zeros_like(Pm)
    F0 = 0.04 + metal * (albedo - 0.04)
    a2 = (rough * rough) ** 2
    k = (rough + 1) ** 2 / 8
    ndv = np.maximum(np.sum(Nn * V, -1, keepdims=True), 0)
    for l, (lc, lp, li) in enumerate(lights):
        lc, lp = np.asarray(lc, float), np.asarray(lp, float)
        sl = s[l, model][:, None]
        L = _norm(lp - Pm)
        cd += albedo * lc * np.maximum(0.0, np.sum(nm * -L, -1, keepdims=True) * li) * sl
        Hh = _norm(V + L)
        dist = np.linalg.norm(lp - Pm, axis=-1, keepdims=True)
        rad = lc / np.maximum(dist * dist, 1.0)
        x = np.clip(1.0 - np.maximum(np.sum(Hh * V, -1, keepdims=True), 0.0), 0, 1)
        F = F0 + (1 - F0) * x ** 5
        ndh = np.maximum(np.sum(Nn * Hh, -1, keepdims=True), 0)
        den = ndh * ndh * (a2 - 1) + 1
        NDF = a2 / (PI * den * den)
        ndl = np.maximum(np.sum(Nn * L, -1, keepdims=True), 0)
        G = (ndl / (ndl * (1 - k) + k)) * (ndv / (ndv * (1 - k) + k))
        spec = NDF * G * F / (4 * ndv * ndl + 0.0001)
        kD = (1 - F) * (1 - metal)
        L0 += (kD * albedo / PI + spec) * rad * ndl * sl
    c = L0 * 0.2
    c = c / (c + 1)
    col = cd + c ** (1 / 2.2)
    if refl is not None:
        r = np.asarray(refl, np.float64).reshape(n, 4)[model, :3]
        on = (reflectivity != 0) & normal_valid(normal[model])
        col[on] = col[on] + reflectivity[on, None] * (r[on] - col[on])
    out[model] = col
    return out
