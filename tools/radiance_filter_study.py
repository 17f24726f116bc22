#!/usr/bin/env python3
"""What the radiance filter costs and what it buys: rt_radiance_accumulate and rt_radiance_atrous at
1920 x 1080 from the library's own planes (C2F's G-buffer, motion and rough reflection plane).

In one process, in interleaved rounds (every case once per round), HIP events around each case on a stream of its own,
medians with p10 / p90 over the rounds after a warm-up:
  copy                    a device-to-device copy of eight 4-float planes' worth of bytes (265 MB read, 265 MB written: a
                          single plane's copy is mostly launch latency): the copy rate every byte floor below is taken
                          at, measured in the same rounds
  accumulate              one launch onto a previous frame of the same camera; floor 128 B per pixel (six 16-byte
                          entries read, two written)
  atrous_<form>_it<k>     rt_radiance_atrous with k = 1 .. 5 iterations under RT_ATROUS_FORM = direct and lds (a
                          context each); step s = 2^(k-1) costs it<k> - it<k-1>, taken round by round; floor 56 B per
                          pixel and iteration (16 + 16 + 4 read, 16 + 4 written). The winner per step (its p90 below
                          the other's p10) is what launch_radiance_atrous's automatic rule is written from
  atrous_auto_it3         three iterations under the library's own rule
  ao_route_it3            what a caller could do before: four rt_ao_atrous runs of three iterations over the four
                          de-interleaved channels (existing entry points only; the de-interleave and re-interleave
                          copies are not timed, and no luminance or variance term exists there)
  refl_S1, refl_S8        rt_dispatch_reflection alone at the study's roughness
  pipeline                rt_dispatch_reflection at S = 1, guide, accumulate, three a-trous iterations, one block

Quality, once per scene (C2F at 1920 x 1080 and REFLO at 1280 x 720): RGB RMSE against an S = 64 plane (its own seed)
of S = 1 raw, S = 8 raw, S = 1 accumulated over 16 static frames, the same after three a-trous iterations, and one S = 1
frame filtered without history.

  python tools/radiance_filter_study.py --launches 100 --out profiles/radiance_filter_study.json
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

FORMS = ("direct", "lds")
ROUGH = 0.3
ATROUS_BYTES, ACC_BYTES, COPY_BYTES = 56, 128, 8 * 32
W, H = 1920, 1080


def context(form, spec):
    if form is not None:
        os.environ["RT_ATROUS_FORM"] = form
    try:
        c = rt.Context(0)
    finally:
        os.environ.pop("RT_ATROUS_FORM", None)
    c.set_motion_history(True)
    scenes.upload(c, spec)
    return c


def f4(n):
    return torch.zeros((n, 4), dtype=torch.float32, device="cuda")


def f1(n):
    return torch.zeros((n,), dtype=torch.float32, device="cuda")


def quality(name, W, H, ts):
    """RGB RMSE against S = 64 on the pixels with a surface, for one scene at its sibling studies' size."""
    spec = scenes.config(name).with_size(W, H)
    n, s = W * H, ts.cuda_stream
    c = context(None, spec)
    hits, normal, motion, guide = torch.zeros((n, 4), dtype=torch.int32, device="cuda"), f4(n), f4(n), f4(n)
    c.dispatch_gbuffer_motion(W, H, hits=hits, normal=normal, motion=motion, stream=s)
    c.denoise_guide(n, normal, motion.view(-1)[3:], guide, stream=s)
    truth, raw1, raw8, one = f4(n), f4(n), f4(n), f4(n)
    c.dispatch_reflection(W, H, truth, 64, ROUGH, seed=1000, stream=s)
    c.dispatch_reflection(W, H, raw1, 1, ROUGH, seed=0, stream=s)
    c.dispatch_reflection(W, H, raw8, 8, ROUGH, seed=0, stream=s)
    pr, pm, qr, qm = f4(n), f4(n), f4(n), f4(n)
    for k in range(16):
        c.dispatch_reflection(W, H, one, 1, ROUGH, seed=k, stream=s)
        if k == 0:
            c.radiance_accumulate(W, H, one, motion, guide, pr, pm, stream=s)
        else:
            c.radiance_accumulate(W, H, one, motion, guide, qr, qm, pr, pm, guide, stream=s)
            pr, pm, qr, qm = qr, qm, pr, pm
    flt, var, tmp, vtmp = f4(n), f1(n), f4(n), f1(n)
    c.radiance_atrous(W, H, pr, pm, guide, flt, var, tmp, vtmp, iterations=3, stream=s)
    nohist, m0 = f4(n), f4(n)
    c.radiance_accumulate(W, H, raw1, motion, guide, qr, m0, stream=s)
    c.radiance_atrous(W, H, qr, m0, guide, nohist, var, tmp, vtmp, iterations=3, stream=s)
    ts.synchronize()
    surface = guide[:, 3] != 0
    t64 = truth.double()[:, :3]

    def rmse(x):
        return float(torch.sqrt(torch.mean((x.double()[:, :3][surface] - t64[surface]) ** 2)))

    out = {"reference": "S = 64, seed 1000", "roughness": ROUGH, "width": W, "height": H,
           "pixels_with_a_surface": int(surface.sum()),
           "rmse_S1_raw": rmse(raw1), "rmse_S8_raw": rmse(raw8), "rmse_S1_accumulated_16": rmse(pr),
           "rmse_S1_accumulated_16_atrous_3": rmse(flt), "rmse_S1_atrous_3_no_history": rmse(nohist)}
    out["filtered_closer_than_S8"] = out["rmse_S1_accumulated_16_atrous_3"] < out["rmse_S8_raw"]
    c.forget_stream(s)
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.launches < 100:
        sys.exit("radiance_filter_study: at least 100 timed rounds")
    if not torch.cuda.is_available():
        sys.exit("radiance_filter_study: needs the GPU (nothing is measured without one)")
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    qual = {name: quality(name, w, h, ts) for name, w, h in (("C2F", 1920, 1080), ("REFLO", 1280, 720))}

    spec = scenes.config("C2F").with_size(W, H)
    n = W * H
    ctx = {f: context(f, spec) for f in FORMS}
    ctx["auto"] = context(None, spec)
    c0 = ctx["auto"]
    hits, normal, motion, guide = torch.zeros((n, 4), dtype=torch.int32, device="cuda"), f4(n), f4(n), f4(n)
    rad, rad8, prev_rad, prev_mom, acc, mom = f4(n), f4(n), f4(n), f4(n), f4(n), f4(n)
    flt, var, tmp, vtmp, copy_src, copy_dst = f4(n), f1(n), f4(n), f1(n), f4(8 * n), f4(8 * n)
    chan, chan_out, chan_tmp = [f1(n) for _ in range(4)], [f1(n) for _ in range(4)], f1(n)
    c0.dispatch_gbuffer_motion(W, H, hits=hits, normal=normal, motion=motion, stream=s)
    c0.denoise_guide(n, normal, motion.view(-1)[3:], guide, stream=s)
    c0.dispatch_reflection(W, H, rad, 1, ROUGH, seed=1, stream=s)
    c0.radiance_accumulate(W, H, rad, motion, guide, prev_rad, prev_mom, stream=s)
    c0.dispatch_reflection(W, H, rad, 1, ROUGH, seed=0, stream=s)
    ts.synchronize()
    with torch.cuda.stream(ts):
        for k in range(4):
            chan[k].copy_(prev_rad[:, k])
    ts.synchronize()

    def copy():
        with torch.cuda.stream(ts):
            copy_dst.copy_(copy_src)

    def ao_route():
        for k in range(4):
            c0.ao_atrous(W, H, chan[k], guide, chan_out[k], chan_tmp, iterations=3, stream=s)

    def pipeline():
        c0.dispatch_reflection(W, H, rad, 1, ROUGH, seed=0, stream=s)
        c0.denoise_guide(n, normal, motion.view(-1)[3:], guide, stream=s)
        c0.radiance_accumulate(W, H, rad, motion, guide, acc, mom, prev_rad, prev_mom, guide, stream=s)
        c0.radiance_atrous(W, H, acc, mom, guide, flt, var, tmp, vtmp, iterations=3, stream=s)

    runs = {
        "copy": copy,
        "accumulate": lambda: c0.radiance_accumulate(W, H, rad, motion, guide, acc, mom, prev_rad, prev_mom, guide,
                                                     stream=s),
        "accumulate_first_frame": lambda: c0.radiance_accumulate(W, H, rad, motion, guide, acc, mom, stream=s),
        "atrous_auto_it3": lambda: c0.radiance_atrous(W, H, prev_rad, prev_mom, guide, flt, var, tmp, vtmp,
                                                      iterations=3, stream=s),
        "ao_route_it3": ao_route,
        "refl_S1": lambda: c0.dispatch_reflection(W, H, rad, 1, ROUGH, seed=0, stream=s),
        "refl_S8": lambda: c0.dispatch_reflection(W, H, rad8, 8, ROUGH, seed=0, stream=s),
        "pipeline": pipeline,
    }
    for f in FORMS:
        for it in range(1, 6):
            runs[f"atrous_{f}_it{it}"] = lambda c=ctx[f], it=it: c.radiance_atrous(
                W, H, prev_rad, prev_mom, guide, flt, var, tmp, vtmp, iterations=it, stream=s)
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

    copy_ms = float(np.median(ms["copy"]))
    copy_tbs = n * COPY_BYTES / (copy_ms * 1e-3) / 1e12

    def floor_ms(nbytes):
        return n * nbytes / (copy_tbs * 1e12) * 1e3

    def stat(v, nbytes=None):
        v = np.asarray(v, np.float64)
        r = {"ms": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}
        if nbytes:
            r["over_floor"] = r["ms"] / floor_ms(nbytes)
        return r

    timing = {k: stat(v, ACC_BYTES if k.startswith("accumulate") else None) for k, v in ms.items()}
    steps = []
    for it in range(1, 6):
        row = {"step": 1 << (it - 1)}
        for f in FORMS:
            cum = np.asarray(ms[f"atrous_{f}_it{it}"])
            row[f] = stat(cum - (np.asarray(ms[f"atrous_{f}_it{it - 1}"]) if it > 1 else 0.0), ATROUS_BYTES)
        row["lds_over_direct"] = row["lds"]["ms"] / row["direct"]["ms"]
        lo, hi = sorted(FORMS, key=lambda f: row[f]["ms"])
        row["faster"] = lo
        row["winner"] = lo if row[lo]["p90"] < row[hi]["p10"] else None  # beyond both spreads
        steps.append(row)
    row = {"config": spec.name, "width": W, "height": H, "rounds": a.launches, "warmup": a.warmup,
           "roughness": ROUGH, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "copy_rate_TBps": copy_tbs,
           "atrous_floor_bytes_per_pixel": ATROUS_BYTES, "atrous_floor_ms": floor_ms(ATROUS_BYTES),
           "accumulate_floor_bytes_per_pixel": ACC_BYTES, "accumulate_floor_ms": floor_ms(ACC_BYTES),
           "timing": timing, "atrous_steps": steps,
           "radiance_atrous_over_ao_route": timing["atrous_auto_it3"]["ms"] / timing["ao_route_it3"]["ms"],
           "pipeline_over_refl_S8": timing["pipeline"]["ms"] / timing["refl_S8"]["ms"]}
    for c in ctx.values():
        c.forget_stream(s)
        c.close()
    doc = {"timing": row, "quality": qual}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        old = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                old = json.load(f)
        old.update(doc)
        with open(a.out, "w") as f:
            f.write(json.dumps(old, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
