#!/usr/bin/env python3
"""What filtering all of a frame's scalar planes in one launch per pass costs against one launch per plane
(DESIGN §3.22): rt_ao_accumulate_planes / rt_ao_atrous_planes against rt_ao_accumulate / rt_ao_atrous called P times,
on the library's own planes (the G-buffer with motion, rt_dispatch_shadow's visibility planes, the AO plane, the guide).

  REFLO at 1280 x 720   P = 7: six lights and the AO plane (the reference frame loop)
  C2F at 1920 x 1080    P = 2: one light and the AO plane
  REFLO at 1280 x 720   P = 1: what the batched path costs a caller who has one plane

One process; every case once per round, the order shuffled anew each round; HIP events around each case on a stream of
its own; medians over the timed rounds with p10 - p90 and min - max. The per-plane entry points are the baseline, not
the code under test: they are called P times inside one timed block.
  accumulate_{batched,perplane}
  atrous_{batched,perplane}_{direct,lds}_it<k>   k = 1 .. 5 iterations under RT_ATROUS_FORM (a context each); step
                          s = 2^(k-1) costs it<k> - it<k-1>, taken round by round
  pair_{batched,perplane}  accumulate and 3 iterations under the library's own choice of form, as one timed block
  copy                    a device-to-device copy of 256 MiB: the bandwidth reached in the same rounds
Every pass is also given as a multiple of its byte floor at that bandwidth: per pixel 68 P (accumulate) and 24 P (one
iteration) for the per-plane calls, 56 + 12 P and 16 + 8 P batched.

A ratio "exceeds both spreads" when the faster case's p90 lies below the slower case's p10.

  python tools/filter_planes_study.py --rounds 100 --out profiles/filter_planes_study.json
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import realtimeraytracing_gradproject_amd as rt  # noqa: E402
from realtimeraytracing_gradproject_amd import scenes  # noqa: E402

RADIUS, TMIN = 2.0, 0.01
FORMS = ("direct", "lds")
COPY_WORDS = 64 << 20
SCENES = (("REFLO", 1280, 720, None), ("C2F", 1920, 1080, None), ("REFLO", 1280, 720, 1))  # None: lights + AO


def context(form, spec):
    old = os.environ.pop("RT_ATROUS_FORM", None)
    if form is not None:
        os.environ["RT_ATROUS_FORM"] = form
    try:
        c = rt.Context(0)
    finally:
        os.environ.pop("RT_ATROUS_FORM", None)
        if old is not None:
            os.environ["RT_ATROUS_FORM"] = old
    c.set_motion_history(True)
    scenes.upload(c, spec)
    return c


def stat(v):
    v = np.asarray(v, np.float64)
    return {"ms": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)),
            "min": float(v.min()), "max": float(v.max())}


def versus(batched, perplane):
    """batched / perplane, and whether the difference exceeds both p10 - p90 spreads (and both min - max ranges)."""
    lo, hi = (batched, perplane) if batched["ms"] <= perplane["ms"] else (perplane, batched)
    return {"batched_over_perplane": batched["ms"] / perplane["ms"],
            "exceeds_both_spreads": bool(lo["p90"] < hi["p10"]), "ranges_disjoint": bool(lo["max"] < hi["min"]),
            "faster": "batched" if batched["ms"] <= perplane["ms"] else "perplane"}


def study(name, w, h, planes, rounds, warmup, rng):
    spec = scenes.config(name).with_size(w, h)
    n, L = w * h, len(spec.lights)
    P = L + 1 if planes is None else planes
    ctx = {f: context(f, spec) for f in FORMS + (None,)}
    c0 = ctx[None]
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    f1 = lambda k=None: torch.zeros((n,) if k is None else (k, n), dtype=torch.float32, device="cuda")  # noqa: E731
    f4 = lambda: torch.zeros((n, 4), dtype=torch.float32, device="cuda")  # noqa: E731
    hits, normal, motion, guide = torch.zeros((n, 4), dtype=torch.int32, device="cuda"), f4(), f4(), f4()
    vis, ao = f1(L), f1()
    torch.cuda.synchronize()  # the zero fills above ran on torch's default stream
    with torch.cuda.stream(ts):
        c0.dispatch_gbuffer_motion(w, h, hits=hits, normal=normal, motion=motion, stream=s)
        c0.dispatch_shadow(w, h, vis, samples=1, light_radius=0.5, seed=0, stream=s)
        c0.dispatch_ao(w, h, ao, 1, RADIUS, TMIN, 0, stream=s)
        c0.denoise_guide(n, normal, motion.view(-1)[3:], guide, stream=s)
        cur = ([vis[l] for l in range(L)] + [ao])[-P:]  # the last P of: the lights' planes, then the AO plane
        guide_prev = guide.clone()
        prev, hist_prev = [f1() for _ in range(P)], f1()
        c0.ao_accumulate_planes(w, h, cur, motion, guide, prev, hist_prev, stream=s)  # the previous frame: this one
        out, tmp, flt = [f1() for _ in range(P)], [f1() for _ in range(P)], [f1() for _ in range(P)]
        hist = [f1() for _ in range(P)]
        src, dst = torch.zeros(COPY_WORDS, dtype=torch.float32, device="cuda"), \
            torch.zeros(COPY_WORDS, dtype=torch.float32, device="cuda")
    ts.synchronize()

    def acc_batched(c=c0):
        c.ao_accumulate_planes(w, h, cur, motion, guide, out, hist[0], prev, hist_prev, guide_prev, stream=s)

    def acc_perplane(c=c0):
        for p in range(P):
            c.ao_accumulate(w, h, cur[p], motion, guide, out[p], hist[p], prev[p], hist_prev, guide_prev, stream=s)

    def atr_batched(c, it, source=prev):
        c.ao_atrous_planes(w, h, source, guide, flt, tmp, iterations=it, stream=s)

    def atr_perplane(c, it, source=prev):
        for p in range(P):
            c.ao_atrous(w, h, source[p], guide, flt[p], tmp[p], iterations=it, stream=s)

    def copy():
        with torch.cuda.stream(ts):
            dst.copy_(src)

    runs = {"accumulate_batched": acc_batched, "accumulate_perplane": acc_perplane, "copy": copy,
            "pair_batched": lambda: (acc_batched(), atr_batched(c0, 3, out)),
            "pair_perplane": lambda: (acc_perplane(), atr_perplane(c0, 3, out))}
    for f in FORMS:
        for it in range(1, 6):
            runs[f"atrous_batched_{f}_it{it}"] = lambda c=ctx[f], it=it: atr_batched(c, it)
            runs[f"atrous_perplane_{f}_it{it}"] = lambda c=ctx[f], it=it: atr_perplane(c, it)
    ms = {k: [] for k in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    order = list(runs)
    torch.cuda.synchronize()
    for k in range(warmup + rounds):
        rng.shuffle(order)
        for case in order:
            e0.record(ts)
            runs[case]()
            e1.record(ts)
            ts.synchronize()
            if k >= warmup:
                ms[case].append(e0.elapsed_time(e1))
    # the batched calls' planes against the per-plane calls', once more, after all that
    acc_batched()
    atr_batched(c0, 3, out)
    ts.synchronize()
    b = [t.clone() for t in flt] + [hist[0].clone()]
    acc_perplane()
    atr_perplane(c0, 3, out)
    ts.synchronize()
    equal = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(b, flt + [hist[0]]))

    timing = {k: stat(v) for k, v in ms.items()}
    copy_tbs = 2 * 4 * COPY_WORDS / (timing["copy"]["ms"] * 1e-3) / 1e12
    floor = lambda nbytes: n * nbytes / (copy_tbs * 1e12) * 1e3  # noqa: E731  (ms)
    bytes_pp = {"accumulate_batched": 56 + 12 * P, "accumulate_perplane": 68 * P, "atrous_batched": 16 + 8 * P,
                "atrous_perplane": 24 * P}
    res = {"config": name, "width": w, "height": h, "planes": P, "lights": L, "rounds": rounds, "warmup": warmup,
           "batched_equals_perplane_bitwise": bool(equal), "copy_TBps": copy_tbs, "copy": timing["copy"],
           "bytes_per_pixel": bytes_pp}
    acc = {k: dict(timing[f"accumulate_{k}"], over_floor=timing[f"accumulate_{k}"]["ms"] /
                   floor(bytes_pp[f"accumulate_{k}"])) for k in ("batched", "perplane")}
    acc["versus"] = versus(acc["batched"], acc["perplane"])
    res["accumulate"] = acc
    steps = []
    for it in range(1, 6):
        row = {"step": 1 << (it - 1)}
        for kind in ("batched", "perplane"):
            for f in FORMS:
                cum = np.asarray(ms[f"atrous_{kind}_{f}_it{it}"])
                d = cum - (np.asarray(ms[f"atrous_{kind}_{f}_it{it - 1}"]) if it > 1 else 0.0)
                st = stat(d)
                st["over_floor"] = st["ms"] / floor(bytes_pp[f"atrous_{kind}"])
                row[f"{kind}_{f}"] = st
            lo, hi = sorted(FORMS, key=lambda f: row[f"{kind}_{f}"]["ms"])
            row[f"{kind}_lds_over_direct"] = row[f"{kind}_lds"]["ms"] / row[f"{kind}_direct"]["ms"]
            row[f"{kind}_form_beyond_spreads"] = lo if row[f"{kind}_{lo}"]["p90"] < row[f"{kind}_{hi}"]["p10"] else None
        # each side in its better form at this step
        best = {kind: min((row[f"{kind}_{f}"] for f in FORMS), key=lambda r: r["ms"]) for kind in ("batched", "perplane")}
        row["versus_best_forms"] = versus(best["batched"], best["perplane"])
        steps.append(row)
    res["atrous_steps"] = steps
    pair = {k: timing[f"pair_{k}"] for k in ("batched", "perplane")}
    pair["versus"] = versus(pair["batched"], pair["perplane"])
    res["pair_3_iterations"] = pair
    for c in ctx.values():
        c.forget_stream(s)
        c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.rounds < 100:
        sys.exit("filter_planes_study: at least 100 timed rounds")
    if not torch.cuda.is_available():
        sys.exit("filter_planes_study: needs the GPU (nothing is measured without one)")
    rng = random.Random(a.seed)
    doc = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "scenes": []}
    for name, w, h, planes in SCENES:
        doc["scenes"].append(study(name, w, h, planes, a.rounds, a.warmup, rng))
        print(json.dumps({k: v for k, v in doc["scenes"][-1].items() if k != "atrous_steps"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
