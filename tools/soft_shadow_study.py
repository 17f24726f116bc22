#!/usr/bin/env python3
"""What the soft-shadow passes (rt_dispatch_shadow, rt_shade_resolve) cost beside the routes a caller had before them
(DESIGN §3.13).

On C2 (teapot + plane, one light, 1920 x 1080) and REF (the reference scene, six lights, 1280 x 720) in one process,
interleaved launch by launch, HIP events around each launch (or group of launches) on a stream of its own, medians
(with p10 / p90) over the rounds after a warm-up, default (packet) schedule:
  shadow    rt_dispatch_shadow: one launch, 4 B per pixel and light stored; S = 1 at radius 0 (the frame's hard
            shadow) and S in {1, 4, 8} at --radius (penumbrae)
  unfused   rt_dispatch_gbuffer with hits + normal + object (40 B per pixel stored), plus rt_trace_rays' any-hit search
            over the S rays of every lit pixel-light pair, already resident on the device (32 B per ray read, 16 B per
            ray stored). The rays are rt.host_shadow_rays' (the pass's own rays); their generation and upload and the
            final reduction are NOT timed, which favours this route
  resolve   rt_shade_resolve with visibility planes, an AO plane and the RGBA8 output, against its byte floor: 16 + 16 +
            8 + 4 nlights + 4 B read and 16 + 4 B written per pixel, over the time
  deferred  rt_dispatch_gbuffer + rt_dispatch_shadow (radius 0, S = 1) + rt_shade_resolve (no AO plane), three
            launches timed as one group, against
  frame     one rt_dispatch_rays frame in RT_SHADE_LAMBERT_SHADOW at one sample per pixel, which the deferred route
            reproduces bit for bit (it walks the same rays and moves planes besides: what the flexibility costs).
--ab-library times the shadow launches of a second build of the library (a code-shape variant,
tools/build_variant.sh: e.g. -DRT_SHADOW_PLAIN_SGPRS=0) in the same rounds, as ab_shadow_*, and reports ab / shipped.

--out keeps what the file already holds: the run's result replaces the file's "timing" section, beside sections
written by hand such as the kernels' resource usage.

  python tools/soft_shadow_study.py --launches 100 --out profiles/shadow_study.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import realtimeraytracing_gradproject_amd as rt  # noqa: E402
from realtimeraytracing_gradproject_amd import scenes  # noqa: E402
import oracle  # noqa: E402  (camera_rays: the frame's camera rays, for host_shadow_rays)

SAMPLES = (1, 4, 8)
TMIN = 0.01
CONFIGS = (("C2", 1920, 1080), ("REF", 1280, 720))
CHUNK_ROWS = 60  # rows of the frame per host_shadow_rays call (its output is n x nlights x S x 32 B of host memory)


def lit_rays(spec, hits, normal, obj, samples, radius):
    """The rays of every lit pixel-light pair, (pairs, samples, 8) on the device, built in row chunks on the host."""
    w, h = spec.width, spec.height
    parts = []
    for y0 in range(0, h, CHUNK_ROWS):
        y1 = min(h, y0 + CHUNK_ROWS)
        sel = slice(y0 * w, y1 * w)
        py, px = np.divmod(np.arange(y0 * w, y1 * w, dtype=np.uint32), np.uint32(w))
        cam = oracle.camera_rays(spec.camera_buffer(), w, h, px, py)
        rays, lit = rt.host_shadow_rays(cam, hits[sel, 0].view(np.float32), normal[sel], obj[sel, 1], px, py,
                                        spec.lights, samples, radius, TMIN)
        live = (lit == 1) & (hits[sel, 3] == 1)[:, None]
        parts.append(torch.from_numpy(np.ascontiguousarray(rays[live])).cuda())
    return torch.cat(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--ab-library", default="", help="a second librtamd.so whose shadow launches are timed alongside")
    ap.add_argument("--out", default="", help="also merge the result into this JSON file under \"timing\" "
                                              "(profiles/shadow_study.json); its other sections are kept")
    a = ap.parse_args()
    if a.launches < 100:
        sys.exit("soft_shadow_study: at least 100 timed launches")
    if not torch.cuda.is_available():
        sys.exit("soft_shadow_study: needs the GPU (nothing is measured without one)")
    ts = torch.cuda.Stream()  # a stream of its own: a null stream handle would mean the context's stream
    s = ts.cuda_stream
    ab = rt._load(a.ab_library) if a.ab_library else None
    cases = [(1, 0.0)] + [(S, a.radius) for S in SAMPLES]
    runs, info, ctxs, keep = {}, {}, [], []
    for name, w, h in CONFIGS:
        spec = scenes.config(name).with_size(w, h)
        n, nl = w * h, len(spec.lights)
        c = rt.Context(0)
        scenes.upload(c, spec)
        c.set_shading(spec.lights, spec.material, rt.RT_SHADE_LAMBERT_SHADOW, 1)
        ctxs.append(c)
        hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        nrm = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        obj = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        vis = torch.zeros((nl * n,), dtype=torch.float32, device="cuda")
        ao = torch.ones((n,), dtype=torch.float32, device="cuda")
        color = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        rgba8 = torch.zeros((n,), dtype=torch.int32, device="cuda")
        f8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        f32 = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        keep += [hits, nrm, obj, vis, ao, color, rgba8, f8, f32]

        # the unfused route's rays: from the library's own planes, once per radius, at the largest S
        c.dispatch_gbuffer(w, h, hits=hits, normal=nrm, object=obj, stream=s)
        ts.synchronize()
        hh, nn, oo = hits.cpu().numpy().view(np.uint32), nrm.cpu().numpy(), obj.cpu().numpy().view(np.uint32)
        hard = lit_rays(spec, hh, nn, oo, 1, 0.0)
        soft = lit_rays(spec, hh, nn, oo, max(SAMPLES), a.radius)
        pairs = int(hard.shape[0])
        assert int(soft.shape[0]) == pairs  # the lit rule does not depend on the radius
        rec = torch.zeros((pairs * max(SAMPLES), 4), dtype=torch.int32, device="cuda")
        keep.append(rec)
        info[name] = {"width": w, "height": h, "pixels": n, "lights": nl, "lit_pairs": pairs,
                      "resolve_bytes": n * (16 + 16 + 8 + 4 * nl + 4 + 16 + 4)}

        def gbuffer(c=c, w=w, h=h, hits=hits, nrm=nrm, obj=obj):
            c.dispatch_gbuffer(w, h, hits=hits, normal=nrm, object=obj, stream=s)

        def resolve(with_ao, c=c, w=w, h=h, hits=hits, nrm=nrm, obj=obj, vis=vis, ao=ao, color=color, rgba8=rgba8):
            c.shade_resolve(w, h, hits, nrm, obj, color, vis=vis, ao=ao if with_ao else None, rgba8_out=rgba8, stream=s)

        def deferred(c=c, w=w, h=h, vis=vis, gbuffer=gbuffer, resolve=resolve):
            gbuffer()
            c.dispatch_shadow(w, h, vis, 1, 0.0, TMIN, stream=s)
            resolve(False)

        cab = None
        if ab is not None:
            cab = rt.Context(0, library=ab)
            scenes.upload(cab, spec)
            ctxs.append(cab)
        runs[f"gbuffer_{name}"] = gbuffer
        for S, radius in cases:
            key = f"{name}_S{S}_r{radius:g}"
            runs[f"shadow_{key}"] = lambda c=c, w=w, h=h, vis=vis, S=S, radius=radius: \
                c.dispatch_shadow(w, h, vis, S, radius, TMIN, stream=s)
            r = (hard if radius == 0.0 else soft[:, :S]).reshape(-1, 8).clone()  # a contiguous copy of its own
            keep.append(r)
            runs[f"trace_{key}"] = lambda c=c, r=r, rec=rec: c.trace_rays(r, r.shape[0], True, rec, stream=s)
            if cab is not None:
                runs[f"ab_shadow_{key}"] = lambda cab=cab, w=w, h=h, vis=vis, S=S, radius=radius: \
                    cab.dispatch_shadow(w, h, vis, S, radius, TMIN, stream=s)
        del hard, soft
        runs[f"resolve_{name}"] = lambda resolve=resolve: resolve(True)
        runs[f"deferred_{name}"] = deferred
        runs[f"frame_{name}"] = lambda c=c, w=w, h=h, f8=f8, f32=f32: c.dispatch(w, h, f8, f32, stream=s)

    ms = {k: [] for k in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    for k in range(a.warmup + a.launches):
        for name, fn in runs.items():
            e0.record(ts)
            fn()
            e1.record(ts)
            ts.synchronize()
            if k >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))

    def stat(v):
        v = np.asarray(v, np.float64)
        return {"ms": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}

    t = {k: stat(v) for k, v in ms.items()}
    row = {"launches": a.launches, "warmup": a.warmup, "tmin": TMIN, "radius": a.radius,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "ab_library": a.ab_library or None, "timing": t, "configs": []}
    for name, _, _ in CONFIGS:
        cfg = dict(info[name], config=name, cases=[])
        g = t[f"gbuffer_{name}"]
        for S, radius in cases:
            key = f"{name}_S{S}_r{radius:g}"
            f, tr = t[f"shadow_{key}"], t[f"trace_{key}"]
            case = {"samples": S, "radius": radius, "rays": cfg["lit_pairs"] * S, "shadow_ms": f["ms"],
                    "unfused_ms": g["ms"] + tr["ms"], "shadow_over_unfused": f["ms"] / (g["ms"] + tr["ms"]),
                    # the ratio with each side at the unfavourable end of its p10-p90 spread, and at the favourable end
                    "shadow_over_unfused_worst": f["p90"] / (g["p10"] + tr["p10"]),
                    "shadow_over_unfused_best": f["p10"] / (g["p90"] + tr["p90"])}
            if ab is not None:
                case["ab_shadow_ms"] = t[f"ab_shadow_{key}"]["ms"]
                case["ab_over_shadow"] = case["ab_shadow_ms"] / f["ms"]
            cfg["cases"].append(case)
        r, d, fr = t[f"resolve_{name}"], t[f"deferred_{name}"], t[f"frame_{name}"]
        cfg["resolve_ms"] = r["ms"]
        cfg["resolve_bytes_per_second"] = cfg["resolve_bytes"] / (r["ms"] * 1e-3)
        cfg["deferred_ms"], cfg["frame_ms"] = d["ms"], fr["ms"]
        cfg["deferred_over_frame"] = d["ms"] / fr["ms"]
        cfg["deferred_over_frame_worst"] = d["p90"] / fr["p10"]
        cfg["deferred_over_frame_best"] = d["p10"] / fr["p90"]
        row["configs"].append(cfg)
    for c in ctxs:
        c.forget_stream(s)
        c.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["timing"] = row
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
