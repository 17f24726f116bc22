#!/usr/bin/env python3
"""What the AO filter costs and what it buys: rt_denoise_guide, rt_ao_accumulate and rt_ao_atrous on C2
(teapot + plane, 1920 x 1080) from the library's own planes.

In one process, in interleaved rounds (every case once per round), HIP events around each case on a stream of its own,
medians with p10 / p90 over the rounds after a warm-up:
  guide, accumulate       one launch each (the accumulate pass reprojects onto a previous frame of the same camera)
  atrous_<form>_it<k>     rt_ao_atrous with k = 1 .. 5 iterations under RT_ATROUS_FORM = direct and lds (a context
                          each); step s = 2^(k-1) costs it<k> - it<k-1>, taken round by round so that the spread is the
                          spread of the difference
  pipeline_<form>         rt_dispatch_ao at S = 1, guide, accumulate, 3 a-trous iterations, as one timed block
  ao_S1, ao_S8            rt_dispatch_ao alone, timed in the same rounds
Each pass is reported against the floor of 24 B per pixel and iteration (16 + 4 read, 4 written) at the 6.29 TB/s copy
rate measured on this part: 7.9 us at 1080p.

Quality, once: RMSE against an S = 64 plane (its own seed) of S = 1 raw, S = 1 accumulated over 16 static frames, the
same after 3 a-trous iterations, and S = 8 raw.

--out keeps what the file already holds: the run replaces its "timing" and "quality" sections, beside sections written
by hand such as the kernels' resource usage.

  python tools/denoise_study.py --launches 100 --out profiles/denoise_study.json
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

RADIUS, TMIN = 2.0, 0.01
FORMS = ("direct", "lds")
COPY_TBS = 6.29
FLOOR_BYTES = 24


def context(form, spec=None):
    os.environ["RT_ATROUS_FORM"] = form
    try:
        c = rt.Context(0)
    finally:
        del os.environ["RT_ATROUS_FORM"]
    if spec is not None:
        c.set_motion_history(True)
        scenes.upload(c, spec)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="C2")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.launches < 100:
        sys.exit("denoise_study: at least 100 timed rounds")
    if not torch.cuda.is_available():
        sys.exit("denoise_study: needs the GPU (nothing is measured without one)")
    spec = scenes.config(a.config)
    w, h, n = spec.width, spec.height, spec.width * spec.height
    ctx = {f: context(f, spec) for f in FORMS}
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    f1 = lambda: torch.zeros((n,), dtype=torch.float32, device="cuda")  # noqa: E731
    f4 = lambda: torch.zeros((n, 4), dtype=torch.float32, device="cuda")  # noqa: E731
    hits, normal, motion = torch.zeros((n, 4), dtype=torch.int32, device="cuda"), f4(), f4()
    guide, ao, acc, hist, flt, tmp = f4(), f1(), f1(), f1(), f1(), f1()
    prev_ao, prev_hist = f1(), f1()
    c0 = ctx[FORMS[0]]
    c0.dispatch_gbuffer_motion(w, h, hits=hits, normal=normal, motion=motion, stream=s)
    c0.dispatch_ao(w, h, ao, 1, RADIUS, TMIN, 0, stream=s)
    c0.denoise_guide(n, normal, motion.view(-1)[3:], guide, stream=s)
    c0.ao_accumulate(w, h, ao, motion, guide, prev_ao, prev_hist, stream=s)
    ts.synchronize()

    # ---- quality ---------------------------------------------------------------------------------------------------
    truth, raw8 = f1(), f1()
    c0.dispatch_ao(w, h, truth, 64, RADIUS, TMIN, 1000, stream=s)
    c0.dispatch_ao(w, h, raw8, 8, RADIUS, TMIN, 0, stream=s)
    pa, ph, qa, qh = f1(), f1(), f1(), f1()
    one = f1()
    for k in range(16):
        c0.dispatch_ao(w, h, one, 1, RADIUS, TMIN, k, stream=s)
        if k == 0:
            c0.ao_accumulate(w, h, one, motion, guide, pa, ph, stream=s)
        else:
            c0.ao_accumulate(w, h, one, motion, guide, qa, qh, pa, ph, guide, stream=s)
            pa, ph, qa, qh = qa, qh, pa, ph
    c0.ao_atrous(w, h, pa, guide, flt, tmp, iterations=3, stream=s)
    ts.synchronize()
    surface = (guide[:, 3] != 0)
    t64 = truth.double()

    def rmse(x):
        return float(torch.sqrt(torch.mean((x.double()[surface] - t64[surface]) ** 2)))

    quality = {"reference": "S = 64, seed 1000", "pixels_with_a_surface": int(surface.sum()),
               "rmse_S1_raw": rmse(ao), "rmse_S1_accumulated_16": rmse(pa), "rmse_S1_accumulated_16_atrous_3": rmse(flt),
               "rmse_S8_raw": rmse(raw8)}
    one_filtered = f1()
    c0.ao_atrous(w, h, ao, guide, one_filtered, tmp, iterations=3, stream=s)
    ts.synchronize()
    quality["rmse_S1_atrous_3_no_history"] = rmse(one_filtered)

    # ---- timing ----------------------------------------------------------------------------------------------------
    runs = {
        "guide": lambda: c0.denoise_guide(n, normal, motion.view(-1)[3:], guide, stream=s),
        "accumulate": lambda: c0.ao_accumulate(w, h, ao, motion, guide, acc, hist, prev_ao, prev_hist, guide, stream=s),
        "ao_S1": lambda: c0.dispatch_ao(w, h, ao, 1, RADIUS, TMIN, 0, stream=s),
        "ao_S8": lambda: c0.dispatch_ao(w, h, raw8, 8, RADIUS, TMIN, 0, stream=s),
    }
    for f in FORMS:
        c = ctx[f]
        for it in range(1, 6):
            runs[f"atrous_{f}_it{it}"] = lambda c=c, it=it: c.ao_atrous(w, h, prev_ao, guide, flt, tmp, iterations=it,
                                                                        stream=s)

        def pipeline(c=c):
            c.dispatch_ao(w, h, ao, 1, RADIUS, TMIN, 0, stream=s)
            c.denoise_guide(n, normal, motion.view(-1)[3:], guide, stream=s)
            c.ao_accumulate(w, h, ao, motion, guide, acc, hist, prev_ao, prev_hist, guide, stream=s)
            c.ao_atrous(w, h, acc, guide, flt, tmp, iterations=3, stream=s)
        runs[f"pipeline_{f}"] = pipeline
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

    floor_ms = n * FLOOR_BYTES / (COPY_TBS * 1e12) * 1e3

    def stat(v):
        v = np.asarray(v, np.float64)
        return {"ms": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)),
                "over_floor": float(np.median(v)) / floor_ms}

    timing = {k: stat(v) for k, v in ms.items()}
    steps = []
    for it in range(1, 6):
        row = {"step": 1 << (it - 1)}
        for f in FORMS:
            cum = np.asarray(ms[f"atrous_{f}_it{it}"])
            d = cum - (np.asarray(ms[f"atrous_{f}_it{it - 1}"]) if it > 1 else 0.0)
            row[f] = stat(d)
        row["lds_over_direct"] = row["lds"]["ms"] / row["direct"]["ms"]
        # beyond the spread: the faster form's p90 below the slower form's p10
        lo, hi = sorted(FORMS, key=lambda f: row[f]["ms"])
        row["winner"] = lo if row[lo]["p90"] < row[hi]["p10"] else None
        steps.append(row)
    row = {"config": spec.name, "width": w, "height": h, "rounds": a.launches, "warmup": a.warmup, "radius": RADIUS,
           "tmin": TMIN, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "floor_bytes_per_pixel": FLOOR_BYTES,
           "copy_rate_TBps": COPY_TBS, "floor_ms": floor_ms, "timing": timing, "atrous_steps": steps}
    for f in FORMS:
        row[f"pipeline_{f}_over_ao_S8"] = timing[f"pipeline_{f}"]["ms"] / timing["ao_S8"]["ms"]
    for c in ctx.values():
        c.forget_stream(s)
        c.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["timing"] = row
        doc["quality"] = quality
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"timing": row, "quality": quality}))


if __name__ == "__main__":
    main()
