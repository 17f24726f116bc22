#!/usr/bin/env python3
"""What the PBR reflection pass (rt_dispatch_reflection_pbr) costs beside the unchanged grey pass
(rt_dispatch_reflection), which is the yardstick and runs in the same rounds.

tools/reflection_pass_study.py's method: one process, interleaved launch by launch, HIP events around each launch on a
stream of its own, medians (with p10 / p90) over the rounds after a warm-up. On C2F (teapot + plane seen from outside,
one light, 1920 x 1080, two materials) and REFLO (the reference scene seen from outside, six lights, 1280 x 720, four
materials), S = 1 at roughness 0 and S = 4 at --roughness, under both schedules:
  grey     rt_dispatch_reflection: every reflected hit a Lambert-shadow sample, one shadow ray per light it faces
  pbr      rt_dispatch_reflection_pbr, flags 0: plane hits one shadow ray to light 0, model hits no shadow ray and the
           GGX / Smith / Schlick arithmetic per light
  pbr_sm   the same with RT_REFLECT_SHADOW_MODELS: the grey pass's walks on the model hits, plus that arithmetic
Each case states the ratio to the yardstick and whether the two p10 - p90 intervals separate.

  python tools/reflection_pbr_study.py --launches 100 --out profiles/reflection_pbr_study.json
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

TMAX, STMIN = 1000.0, 0.01
MATERIALS = [(1.0, 1.0, 1.0, 0.5, 0.5, 0.0), (0.9, 0.15, 0.1, 0.2, 0.0, 0.0), (0.1, 0.7, 0.25, 0.9, 1.0, 0.0),
             (0.2, 0.3, 0.95, 0.35, 0.75, 0.0)]
# scene, width, height, materials, instance -> material
CONFIGS = (("C2F", 1920, 1080, MATERIALS[:2], [1, 0]), ("REFLO", 1280, 720, MATERIALS, [1, 2, 2, 3, 0, 1, 3]))
VARIANTS = (("grey", None), ("pbr", 0), ("pbr_sm", rt.RT_REFLECT_SHADOW_MODELS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--roughness", type=float, default=0.3)
    ap.add_argument("--out", default="", help="also write the result to this JSON file")
    a = ap.parse_args()
    if a.launches < 100:
        sys.exit("reflection_pbr_study: at least 100 timed launches")
    if not torch.cuda.is_available():
        sys.exit("reflection_pbr_study: needs the GPU (nothing is measured without one)")
    ts = torch.cuda.Stream()  # a stream of its own: a null stream handle would mean the context's stream
    s = ts.cuda_stream
    cases = [(1, 0.0), (4, a.roughness)]
    runs, ctxs, keep = {}, [], []
    for name, w, h, mats, imap in CONFIGS:
        spec = scenes.config(name).with_size(w, h)
        n = w * h
        rad = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        d_map = torch.tensor(imap, dtype=torch.int32, device="cuda")
        keep += [rad, d_map]
        for sched in ("packet", "lane"):
            c = rt.Context(0)
            scenes.upload(c, spec)
            c.set_schedule(rt.RT_SCHED_LANE if sched == "lane" else rt.RT_SCHED_PACKET)
            ctxs.append(c)
            for S, roughness in cases:
                for tag, flags in VARIANTS:
                    key = f"{tag}_{sched}_{name}_S{S}_r{roughness:g}"
                    if flags is None:
                        runs[key] = lambda c=c, w=w, h=h, rad=rad, S=S, roughness=roughness: \
                            c.dispatch_reflection(w, h, rad, S, roughness, TMAX, STMIN, stream=s)
                    else:
                        runs[key] = lambda c=c, w=w, h=h, rad=rad, S=S, roughness=roughness, mats=mats, d_map=d_map, \
                            flags=flags: c.dispatch_reflection_pbr(w, h, rad, mats, d_map, S, roughness, TMAX, STMIN,
                                                                   flags=flags, stream=s)
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
           "timing": t, "cases": []}
    for name, w, h, mats, _ in CONFIGS:
        for sched in ("packet", "lane"):
            for S, roughness in cases:
                g = t[f"grey_{sched}_{name}_S{S}_r{roughness:g}"]
                for tag, flags in VARIANTS[1:]:
                    p = t[f"{tag}_{sched}_{name}_S{S}_r{roughness:g}"]
                    row["cases"].append({"config": name, "width": w, "height": h, "materials": len(mats),
                                         "schedule": sched, "samples": S, "roughness": roughness, "flags": flags,
                                         "grey_ms": g["ms"], "pbr_ms": p["ms"], "pbr_over_grey": p["ms"] / g["ms"],
                                         "intervals_separate": bool(p["p10"] > g["p90"] or p["p90"] < g["p10"])})
    for c in ctxs:
        c.forget_stream(s)
        c.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(row, indent=1) + "\n")
    print(json.dumps(row["cases"]))


if __name__ == "__main__":
    main()
