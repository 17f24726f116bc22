#!/usr/bin/env python3
"""What the reflection pass (rt_dispatch_reflection) and its composite (rt_reflection_composite) cost, beside the route
a caller had before them.

On C2F (teapot + plane seen from outside, one light, 1920 x 1080) and REFLO (the reference scene seen from outside,
six lights, 1280 x 720) in one process, interleaved launch by launch, HIP events around each launch (or group of
launches) on a stream of its own, medians (with p10 / p90) over the rounds after a warm-up. Cases: S = 1 at roughness 0
(the mirror ray), S = 1 and S = 4 at --roughness.
  packet    rt_dispatch_reflection under RT_SCHED_PACKET: one launch, 16 B per pixel stored
  lane      the same under RT_SCHED_LANE (reflection rays off curved surfaces are incoherent: which schedule wins is
            what this measures; there is no automatic switch)
  unfused   existing entry points only, so reproducible on the parent commit: rt_dispatch_gbuffer with hits + normal
            (32 B per pixel stored), plus rt_trace_rays' closest-hit search with back faces culled over the reflection
            rays, plus rt_trace_rays' any-hit search over the shadow rays of the lit (reflected hit, light) pairs, both
            ray sets already resident on the device (32 B per ray read, 16 B per ray stored). The rays are the pass's
            own (rt.host_reflection_rays, rt.host_shadow_rays); their generation and upload, and the shading and the
            reduction, are NOT timed, which favours this route
  composite rt_reflection_composite with the RGBA8 output, against its byte floor: 4 x 16 B read and 16 + 4 B written
            per pixel, over the time
--ab-library times the packet launches of a second build of the library (tools/build_variant.sh, e.g.
-DRT_REFLECT_PLAIN_SGPRS=0) in the same rounds, as ab_*, and reports ab / shipped.

--out keeps what the file already holds: the run's result replaces the file's "timing" section.

  python tools/reflection_pass_study.py --launches 100 --out profiles/reflection_study.json
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
import oracle  # noqa: E402  (camera_rays: the frame's camera rays, for host_reflection_rays)

TMAX, STMIN = 1000.0, 0.01
CONFIGS = (("C2F", 1920, 1080), ("REFLO", 1280, 720))
CHUNK_ROWS = 120  # rows of the frame per host call (the rays are n x S x 32 B of host memory)


def route_rays(c, spec, hits, normal, samples, roughness, s, ts):
    """The unfused route's two resident ray sets, per sample k < samples a pair of device tensors: the valid pixels'
    reflection rays k, (pixels, 8), and the shadow rays of their lit (reflected hit, light) pairs, (pairs, 8). Built in
    row chunks: the reflection rays are traced by the library, their hits' normals come from rt.host_shading_normals,
    the shadow rays from rt.host_shadow_rays with the reflection rays as its camera rays."""
    w, h = spec.width, spec.height
    groups = np.array([hg for (_, _, _, hg) in spec.instances], np.uint32)
    refl = [[] for _ in range(samples)]
    shadow = [[] for _ in range(samples)]
    for y0 in range(0, h, CHUNK_ROWS):
        y1 = min(h, y0 + CHUNK_ROWS)
        sel = slice(y0 * w, y1 * w)
        py, px = np.divmod(np.arange(y0 * w, y1 * w, dtype=np.uint32), np.uint32(w))
        cam = oracle.camera_rays(spec.camera_buffer(), w, h, px, py)
        rays, valid = rt.host_reflection_rays(cam, hits[sel, 0].view(np.float32), normal[sel], px, py, samples,
                                              roughness, TMAX, STMIN)
        live = (valid == 1) & (hits[sel, 3] == 1)
        for k in range(samples):
            r = np.ascontiguousarray(rays[live, k])
            if r.shape[0] == 0:
                continue
            d_r = torch.from_numpy(r).cuda()
            rec = torch.zeros((r.shape[0], 4), dtype=torch.int32, device="cuda")
            uv = torch.zeros((r.shape[0], 2), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            c.trace_rays(d_r, r.shape[0], False, rec, uv, stream=s, cull_back=True)
            ts.synchronize()
            rec, uv = rec.cpu().numpy().view(np.uint32), uv.cpu().numpy()
            found = rec[:, 3] == 1
            hn = np.zeros((r.shape[0], 4), np.float32)
            for i, (m, x, _, hg) in enumerate(spec.instances):
                pick = found & (rec[:, 1] == i)
                if pick.any():
                    v, idx = spec.meshes[m]
                    hn[pick] = rt.host_shading_normals(v, idx, rec[pick, 2], uv[pick], hg, x)
            zero = np.zeros(int(found.sum()), np.uint32)
            srays, lit = rt.host_shadow_rays(r[found], rec[found, 0].view(np.float32), hn[found],
                                             groups[rec[found, 1]], zero, zero, spec.lights, 1, 0.0, STMIN)
            refl[k].append(d_r)
            shadow[k].append(torch.from_numpy(np.ascontiguousarray(srays[:, :, 0][lit == 1])).cuda())
    return [(torch.cat(refl[k]), torch.cat(shadow[k])) for k in range(samples)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--roughness", type=float, default=0.3)
    ap.add_argument("--ab-library", default="", help="a second librtamd.so whose packet launches are timed alongside")
    ap.add_argument("--out", default="", help="also merge the result into this JSON file under \"timing\" "
                                              "(profiles/reflection_study.json); its other sections are kept")
    a = ap.parse_args()
    if a.launches < 100:
        sys.exit("reflection_pass_study: at least 100 timed launches")
    if not torch.cuda.is_available():
        sys.exit("reflection_pass_study: needs the GPU (nothing is measured without one)")
    ts = torch.cuda.Stream()  # a stream of its own: a null stream handle would mean the context's stream
    s = ts.cuda_stream
    ab = rt._load(a.ab_library) if a.ab_library else None
    cases = [(1, 0.0), (1, a.roughness), (4, a.roughness)]
    runs, info, ctxs, keep = {}, {}, [], []
    for name, w, h in CONFIGS:
        spec = scenes.config(name).with_size(w, h)
        n = w * h
        ctx = {}
        for sched, lib in (("packet", None), ("lane", None), ("ab", ab)):
            if sched == "ab" and ab is None:
                continue
            c = rt.Context(0, library=lib) if lib is not None else rt.Context(0)
            scenes.upload(c, spec)
            c.set_schedule(rt.RT_SCHED_LANE if sched == "lane" else rt.RT_SCHED_PACKET)
            ctx[sched] = c
            ctxs.append(c)
        c = ctx["packet"]
        hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        nrm = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        rad = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        color = torch.full((n, 4), 0.5, dtype=torch.float32, device="cuda")
        out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        rgba8 = torch.zeros((n,), dtype=torch.int32, device="cuda")
        keep += [hits, nrm, rad, color, out, rgba8]
        torch.cuda.synchronize()
        c.dispatch_gbuffer(w, h, hits=hits, normal=nrm, stream=s)
        ts.synchronize()
        hh, nn = hits.cpu().numpy().view(np.uint32), nrm.cpu().numpy()
        mirror = route_rays(c, spec, hh, nn, 1, 0.0, s, ts)
        rough = route_rays(c, spec, hh, nn, 4, a.roughness, s, ts)
        valid = int(mirror[0][0].shape[0])
        info[name] = {"width": w, "height": h, "pixels": n, "lights": len(spec.lights), "valid_pixels": valid,
                      "composite_bytes": n * (4 * 16 + 16 + 4)}

        def gbuffer(c=c, w=w, h=h, hits=hits, nrm=nrm):
            c.dispatch_gbuffer(w, h, hits=hits, normal=nrm, stream=s)

        runs[f"gbuffer_{name}"] = gbuffer
        for S, roughness in cases:
            key = f"{name}_S{S}_r{roughness:g}"
            for sched, cc in ctx.items():
                runs[f"{sched}_{key}"] = lambda cc=cc, w=w, h=h, rad=rad, S=S, roughness=roughness: \
                    cc.dispatch_reflection(w, h, rad, S, roughness, TMAX, STMIN, stream=s)
            sets = mirror if roughness == 0.0 else rough[:S]
            rr = torch.cat([p[0] for p in sets]).contiguous()
            sr = torch.cat([p[1] for p in sets]).contiguous()
            rec = torch.zeros((max(rr.shape[0], sr.shape[0]), 4), dtype=torch.int32, device="cuda")
            keep += [rr, sr, rec]
            info[name][f"rays_S{S}_r{roughness:g}"] = {"reflection": int(rr.shape[0]), "shadow": int(sr.shape[0])}

            def traces(c=c, rr=rr, sr=sr, rec=rec):
                c.trace_rays(rr, rr.shape[0], False, rec, stream=s, cull_back=True)
                c.trace_rays(sr, sr.shape[0], True, rec, stream=s)

            runs[f"trace_{key}"] = traces
        del mirror, rough
        runs[f"composite_{name}"] = lambda c=c, w=w, h=h, color=color, rad=rad, hits=hits, nrm=nrm, out=out, rgba8=rgba8: \
            c.reflection_composite(w, h, color, rad, hits, nrm, out, 0.8, 0.04, rgba8_out=rgba8, stream=s)

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
    row = {"launches": a.launches, "warmup": a.warmup, "tmax": TMAX, "shadow_tmin": STMIN, "roughness": a.roughness,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "ab_library": a.ab_library or None, "timing": t, "configs": []}
    for name, _, _ in CONFIGS:
        cfg = dict(info[name], config=name, cases=[])
        g = t[f"gbuffer_{name}"]
        for S, roughness in cases:
            key = f"{name}_S{S}_r{roughness:g}"
            p, ln, tr = t[f"packet_{key}"], t[f"lane_{key}"], t[f"trace_{key}"]
            best = min(p, ln, key=lambda x: x["ms"])
            case = {"samples": S, "roughness": roughness, "packet_ms": p["ms"], "lane_ms": ln["ms"],
                    "lane_over_packet": ln["ms"] / p["ms"], "lane_over_packet_worst": ln["p90"] / p["p10"],
                    "lane_over_packet_best": ln["p10"] / p["p90"], "unfused_ms": g["ms"] + tr["ms"],
                    "packet_over_unfused": p["ms"] / (g["ms"] + tr["ms"]),
                    "best_over_unfused": best["ms"] / (g["ms"] + tr["ms"]),
                    # each side at the unfavourable end of its p10-p90 spread, and at the favourable end
                    "best_over_unfused_worst": best["p90"] / (g["p10"] + tr["p10"]),
                    "best_over_unfused_best": best["p10"] / (g["p90"] + tr["p90"])}
            if ab is not None:
                case["ab_ms"] = t[f"ab_{key}"]["ms"]
                case["ab_over_packet"] = case["ab_ms"] / p["ms"]
            cfg["cases"].append(case)
        r = t[f"composite_{name}"]
        cfg["composite_ms"] = r["ms"]
        cfg["composite_bytes_per_second"] = cfg["composite_bytes"] / (r["ms"] * 1e-3)
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
