#!/usr/bin/env python3
"""What the chained PBR reflection pass (rt_dispatch_reflection_chain) costs beside the unchanged one-bounce pass
(rt_dispatch_reflection_pbr), which is the yardstick and runs in the same rounds.

tools/reflection_pbr_study.py's method: one process, interleaved launch by launch, HIP events around each launch on a
stream of its own, medians (with p10 / p90) over the rounds after a warm-up; the order of the launches is shuffled anew
in every round (seeded), so that no variant always follows a change of scene. On C2F (teapot + plane seen from outside,
one light, 1920 x 1080, the teapot reflective) and REFLO (the reference scene seen from outside, six lights,
1280 x 720, the frame anchor's table: instance ids 0 and 1 reflective), one sample at roughness 0 with
RT_REFLECT_FRAME_RAY, under both schedules:
  pbr        rt_dispatch_reflection_pbr: the yardstick
  chain_1    rt_dispatch_reflection_chain, max_bounces 1: the same planes byte for byte, so the difference is the price
             of the chain machinery (the level loop and the scratch-memory stack) where no chain exists
  chain_2, chain_4, chain_18   max_bounces 2, 4 and 18: the chains themselves
and, for orientation, on REFLO
  frame      rt_dispatch_rays in RT_SHADE_REF, which walks the same chains inside the frame kernel (and shades the
             primary hits as well: not the same work, an order of magnitude only).
Each case states the ratio to the yardstick and whether the two p10 - p90 intervals separate. Not measured: the trace
kernels' own times, hardware counters, the frame loop end to end.

  python tools/reflection_chain_study.py --launches 100 --out profiles/reflection_chain_study.json
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
MIRROR = (1.0, 1.0, 1.0, 0.5, 0.5, 0.5)
DULL = MIRROR[:5] + (0.0,)
# scene, width, height, materials, instance -> material
CONFIGS = (("C2F", 1920, 1080, [MIRROR, DULL], [0, 1]), ("REFLO", 1280, 720, [MIRROR, DULL], [0, 0, 1, 1, 1, 1, 1]))
BOUNCES = (1, 2, 4, 18)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the result to this JSON file")
    a = ap.parse_args()
    if a.launches < 100:
        sys.exit("reflection_chain_study: at least 100 timed launches")
    if not torch.cuda.is_available():
        sys.exit("reflection_chain_study: needs the GPU (nothing is measured without one)")
    ts = torch.cuda.Stream()  # a stream of its own: a null stream handle would mean the context's stream
    s = ts.cuda_stream
    flags = rt.RT_REFLECT_FRAME_RAY
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
            runs[f"pbr_{sched}_{name}"] = lambda c=c, w=w, h=h, rad=rad, mats=mats, d_map=d_map: \
                c.dispatch_reflection_pbr(w, h, rad, mats, d_map, 1, 0.0, TMAX, STMIN, flags=flags, stream=s)
            for mb in BOUNCES:
                runs[f"chain_{mb}_{sched}_{name}"] = lambda c=c, w=w, h=h, rad=rad, mats=mats, d_map=d_map, mb=mb: \
                    c.dispatch_reflection_chain(w, h, rad, mats, d_map, 1, 0.0, TMAX, STMIN, flags=flags,
                                                max_bounces=mb, stream=s)
            if name == "REFLO":
                c.set_shading(spec.lights, MIRROR, rt.RT_SHADE_REF, 1)
                out8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
                out32 = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
                keep += [out8, out32]
                runs[f"frame_{sched}_{name}"] = lambda c=c, w=w, h=h, out8=out8, out32=out32: \
                    c.dispatch(w, h, out8, out32, stream=s)
    ms = {k: [] for k in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    order, rng = list(runs.items()), np.random.default_rng(20)
    for k in range(a.warmup + a.launches):
        rng.shuffle(order)  # no launch keeps a fixed predecessor: the first launch after a change of scene pays for it
        for name, fn in order:
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
    row = {"launches": a.launches, "warmup": a.warmup, "tmax": TMAX, "shadow_tmin": STMIN, "samples": 1, "roughness": 0.0,
           "flags": flags, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "timing": t, "cases": []}
    for name, w, h, _, _ in CONFIGS:
        for sched in ("packet", "lane"):
            g = t[f"pbr_{sched}_{name}"]
            tags = [f"chain_{mb}" for mb in BOUNCES] + (["frame"] if name == "REFLO" else [])
            for tag in tags:
                p = t[f"{tag}_{sched}_{name}"]
                row["cases"].append({"config": name, "width": w, "height": h, "schedule": sched, "variant": tag,
                                     "pbr_ms": g["ms"], "ms": p["ms"], "p10": p["p10"], "p90": p["p90"],
                                     "over_pbr": p["ms"] / g["ms"],
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
