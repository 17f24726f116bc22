#!/usr/bin/env python3
"""What the PBR resolve (rt_shade_resolve_pbr) costs beside two yardsticks that are not the code under test (DESIGN
§3.15).

On C2F (teapot + plane seen from outside, one light, two instances, 1920 x 1080) and REFLO (the reference scene seen
from outside, six lights, four materials, 1280 x 720) in one process, interleaved launch by launch, HIP events around
each launch on a stream of its own, medians (with p10 / p90) over the rounds after a warm-up. The planes are the
library's own: rt_dispatch_gbuffer's, rt_dispatch_shadow's (radius 0, one sample), rt_dispatch_ao's and
rt_dispatch_reflection's; every material has reflectivity 0.25, so the radiance plane is read wherever a model is seen.
  pbr_<planes>          rt_shade_resolve_pbr with the RGBA8 output, for every subset of vis, ao and refl
  lambert_<planes>      the unchanged rt_shade_resolve in the same rounds, for every subset of vis and ao (it has no
                        refl input; a case with refl is compared with the same case without it)
  floor                 the bytes the algorithm must move, 60 B per pixel (hits 16, normal 16, object 8, colour 16,
                        RGBA8 4) + 4 per visibility plane + 4 for ao + 16 for refl, at the 6.29 TB/s a float4 copy
                        reaches on this part
The result holds the ratio of each pbr case to both. No pass mark: the kernel evaluates the GGX / Smith / Schlick term
per light where the Lambert resolve takes a dot product, so which bound applies is itself a result.

--out keeps what the file already holds: the run's result replaces the file's "timing" section, beside sections
written by hand such as the kernel's resource usage and the record of the A/B between its two forms.

  python tools/material_resolve_study.py --launches 100 --out profiles/material_study.json
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

COPY_BYTES_PER_SECOND = 6.29e12
MATERIALS = [(1.0, 1.0, 1.0, 0.5, 0.5, 0.25), (0.9, 0.15, 0.1, 0.2, 0.0, 0.25), (0.1, 0.7, 0.25, 0.9, 1.0, 0.25),
             (0.2, 0.3, 0.95, 0.35, 0.75, 0.25)]
# config, width, height, materials, instance -> material
CONFIGS = (("C2F", 1920, 1080, MATERIALS[:2], [1, 0]), ("REFLO", 1280, 720, MATERIALS, [1, 2, 2, 3, 0, 1, 3]))


def label(subset):
    return "+".join(n for k, n in enumerate(("vis", "ao", "refl")) if subset >> k & 1) or "none"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="", help="also merge the result into this JSON file under \"timing\" "
                                              "(profiles/material_study.json); its other sections are kept")
    a = ap.parse_args()
    if a.launches < 100:
        sys.exit("material_resolve_study: at least 100 timed launches")
    if not torch.cuda.is_available():
        sys.exit("material_resolve_study: needs the GPU (nothing is measured without one)")
    ts = torch.cuda.Stream()  # a stream of its own: a null stream handle would mean the context's stream
    s = ts.cuda_stream
    runs, info, ctxs, keep = {}, {}, [], []
    for name, w, h, mats, imap in CONFIGS:
        spec = scenes.config(name).with_size(w, h)
        n, nl = w * h, len(spec.lights)
        c = rt.Context(0)
        scenes.upload(c, spec)
        c.set_shading(spec.lights, spec.material, rt.RT_SHADE_REF, 1)
        ctxs.append(c)
        hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        nrm = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        obj = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        vis = torch.zeros((nl * n,), dtype=torch.float32, device="cuda")
        ao = torch.zeros((n,), dtype=torch.float32, device="cuda")
        refl = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        color = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        rgba8 = torch.zeros((n,), dtype=torch.int32, device="cuda")
        dmap = torch.tensor(imap, dtype=torch.int32, device="cuda")
        keep += [hits, nrm, obj, vis, ao, refl, color, rgba8, dmap]
        torch.cuda.synchronize()
        c.dispatch_gbuffer(w, h, hits=hits, normal=nrm, object=obj, stream=s)
        c.dispatch_shadow(w, h, vis, 1, 0.0, 0.01, stream=s)
        c.dispatch_ao(w, h, ao, 4, 1.0, stream=s)
        c.dispatch_reflection(w, h, refl, stream=s)
        ts.synchronize()
        hit = hits[:, 3] != 0
        model = hit & (obj[:, 1] != rt.RT_HITGROUP_PLANE)
        info[name] = {"width": w, "height": h, "pixels": n, "lights": nl, "materials": len(mats),
                      "instances": len(spec.instances), "hit_pixels": int(hit.sum()), "model_pixels": int(model.sum())}
        for subset in range(8):
            v, o, r = (p if subset >> k & 1 else None for k, p in enumerate((vis, ao, refl)))
            runs[f"pbr_{name}_{label(subset)}"] = \
                lambda c=c, w=w, h=h, hits=hits, nrm=nrm, obj=obj, color=color, mats=mats, dmap=dmap, v=v, o=o, r=r, \
                rgba8=rgba8: c.shade_resolve_pbr(w, h, hits, nrm, obj, color, mats, instance_material=dmap, vis=v, ao=o,
                                                 refl=r, rgba8_out=rgba8, stream=s)
        for subset in range(4):
            v, o = (p if subset >> k & 1 else None for k, p in enumerate((vis, ao)))
            runs[f"lambert_{name}_{label(subset)}"] = \
                lambda c=c, w=w, h=h, hits=hits, nrm=nrm, obj=obj, color=color, v=v, o=o, rgba8=rgba8: \
                c.shade_resolve(w, h, hits, nrm, obj, color, vis=v, ao=o, rgba8_out=rgba8, stream=s)

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
    row = {"launches": a.launches, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "copy_bytes_per_second": COPY_BYTES_PER_SECOND,
           "timing": t, "configs": []}
    for name, _, _, _, _ in CONFIGS:
        cfg = dict(info[name], config=name, cases=[])
        for subset in range(8):
            per_pixel = 60 + (4 * cfg["lights"] if subset & 1 else 0) + (4 if subset & 2 else 0) + (16 if subset & 4 else 0)
            floor_ms = cfg["pixels"] * per_pixel / COPY_BYTES_PER_SECOND * 1e3
            lam = t[f"lambert_{name}_{label(subset & 3)}"]
            case = {"planes": label(subset), "bytes_per_pixel": per_pixel, "floor_ms": floor_ms, "lambert_ms": lam["ms"],
                    "lambert_p10": lam["p10"], "lambert_p90": lam["p90"]}
            p = t[f"pbr_{name}_{label(subset)}"]
            case.update({"pbr_ms": p["ms"], "pbr_p10": p["p10"], "pbr_p90": p["p90"],
                         "pbr_over_lambert": p["ms"] / lam["ms"], "pbr_over_floor": p["ms"] / floor_ms,
                         "pbr_bytes_per_second": cfg["pixels"] * per_pixel / (p["ms"] * 1e-3)})
            cfg["cases"].append(case)
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
    print(json.dumps(row["configs"]))


if __name__ == "__main__":
    main()
