#!/usr/bin/env python3
"""What the temporal upscaler costs: rt_upscale alone in both forms, and the whole route beside a native
frame, on one MI355X.

In one process, in interleaved rounds (every case once per round), HIP events around each case on a stream of its own,
medians with p10 / p90 over the rounds after a warm-up:
  upscale_<form>_<H>   one rt_upscale launch with history and rgba8_out under RT_UPSCALE_FORM = direct and lds (a
                       context each): 960 x 540 -> 1920 x 1080 on C2's planes, 1920 x 1080 -> 3840 x 2160 on C5's. The
                       planes are the library's own: two jittered frames (Halton 0 and 1) with their motion planes.
  upscale_<form>_<w>x<h>_to_1920x1080   the same at the other ratios, 1, 1.5 and 4 per axis, on C2's planes
  route_<config>       rt_dispatch_rays at half the config's size (rgba8 and rgba32f, the config's own spp and mode) +
                       rt_dispatch_gbuffer_motion with `motion` only + rt_upscale (the library's choice of form, with
                       rgba8_out), as one timed block, for C2 and C5
  native_<config>      rt_dispatch_rays at the config's size (rgba8 only), from --yardstick LIB: a build of the parent
                       commit's library, so that the yardstick is code this change cannot have touched (absent: this
                       library, and the file says so)
Each pass is reported against its byte floor at the 6.29 TB/s copy rate §3.10 uses: render-resolution colour and motion
read once (32 B per render pixel), previous colour and history read once (20 B per display pixel), the outputs written
(16 + 4 + 4 B per display pixel). Not in the floor: the previous motion plane's .w (4 B used of each 16 B entry, the
entry under each accepted bilinear tap) and the re-reads of the 3 x 3 taps.

--out keeps what the file already holds: the run replaces its "timing" section, beside sections written by hand such as
the kernels' resource usage and the quality figures measured on the CPU.

  python tools/upscale_study.py --launches 100 --yardstick ab/parent/librtamd.so --out profiles/upscale_study.json
"""
import argparse
import ctypes
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
COPY_TBS = 6.29


def context(form, spec, library=None):
    if form is not None:
        os.environ["RT_UPSCALE_FORM"] = form
    try:
        c = rt.Context(0, library=library)
    finally:
        os.environ.pop("RT_UPSCALE_FORM", None)
    c.set_motion_history(True)
    scenes.upload(c, spec)
    return c


def load_yardstick(path):
    """An older build of the library: the entry points it has, with this module's signatures."""
    lib = ctypes.CDLL(path)
    for name, res, args in rt.SIGNATURES:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--yardstick", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.launches < 100:
        sys.exit("upscale_study: at least 100 timed rounds")
    if not torch.cuda.is_available():
        sys.exit("upscale_study: needs the GPU (nothing is measured without one)")
    yard = load_yardstick(a.yardstick) if a.yardstick else None
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
    runs, sizes, keep, ratios = {}, {}, [], []
    for name in ("C2", "C5"):
        full = scenes.config(name)
        W, H = full.width, full.height
        w, h = W // 2, H // 2
        half = full.with_size(w, h)
        cb0 = half.camera_buffer()
        j0, j1 = rt.jitter_halton(0), rt.jitter_halton(1)
        cbs = [rt.camera_jitter(cb0, w, h, *j0), rt.camera_jitter(cb0, w, h, *j1)]
        ctx = {f: context(f, half) for f in FORMS}
        auto = context(None, half)
        native = context(None, full, yard)
        c0 = ctx[FORMS[0]]
        col = [f32(h, w, 4), f32(h, w, 4)]
        mot = [f32(w * h, 4), f32(w * h, 4)]
        r8 = u8(h, w, 4)
        out, hist, o8 = [f32(W * H, 4), f32(W * H, 4)], [f32(W * H), f32(W * H)], u8(H, W, 4)
        n8 = u8(H, W, 4)
        for k in (0, 1):  # frame 0 without history, frame 1 onto it: the planes every timed launch then reads
            c0.set_camera(cbs[k])
            c0.dispatch(w, h, r8, col[k], stream=s)
            c0.dispatch_gbuffer_motion(w, h, motion=mot[k], prev_camera=cbs[0], stream=s)
        c0.upscale(w, h, W, H, col[0], mot[0], out[0], hist[0], jitter_cur=j0, stream=s)
        ts.synchronize()
        auto.set_camera(cbs[1])
        for f in FORMS:
            runs[f"upscale_{f}_{H}"] = lambda c=ctx[f], w=w, h=h, W=W, H=H, col=col, mot=mot, out=out, hist=hist, o8=o8, \
                j0=j0, j1=j1: c.upscale(w, h, W, H, col[1], mot[1], out[1], hist[1], mot[0], out[0], hist[0],
                                        rgba8_out=o8, jitter_cur=j1, jitter_prev=j0, stream=s)

        def route(c=auto, w=w, h=h, W=W, H=H, col=col, mot=mot, out=out, hist=hist, o8=o8, r8=r8, j0=j0, j1=j1,
                  pcb=cbs[0]):
            c.dispatch(w, h, r8, col[1], stream=s)
            c.dispatch_gbuffer_motion(w, h, motion=mot[1], prev_camera=pcb, stream=s)
            c.upscale(w, h, W, H, col[1], mot[1], out[1], hist[1], mot[0], out[0], hist[0], rgba8_out=o8,
                      jitter_cur=j1, jitter_prev=j0, stream=s)
        runs[f"route_{name}"] = route
        runs[f"native_{name}"] = lambda c=native, W=W, H=H, n8=n8: c.dispatch(W, H, n8, stream=s)
        sizes[name] = dict(render=[w, h], display=[W, H], spp=full.spp,
                           floor_bytes=32 * w * h + (20 + 24) * W * H)
        keep += list(ctx.values()) + [auto, native]
        if name != "C2":
            continue
        # the other ratios at C2's display size: 1, 1.5 and 4 per axis (frames and motion planes rendered the same way)
        for rw, rh in ((W, H), (2 * W // 3, 2 * H // 3), (W // 4, H // 4)):
            spec = full.with_size(rw, rh)
            rcb = [rt.camera_jitter(spec.camera_buffer(), rw, rh, *j0), rt.camera_jitter(spec.camera_buffer(), rw, rh, *j1)]
            rcol, rmot, rr8 = [f32(rh, rw, 4), f32(rh, rw, 4)], [f32(rw * rh, 4), f32(rw * rh, 4)], u8(rh, rw, 4)
            for k in (0, 1):
                c0.set_camera(rcb[k])
                c0.dispatch(rw, rh, rr8, rcol[k], stream=s)
                c0.dispatch_gbuffer_motion(rw, rh, motion=rmot[k], prev_camera=rcb[0], stream=s)
            ts.synchronize()
            for f in FORMS:
                runs[f"upscale_{f}_{rw}x{rh}_to_{W}x{H}"] = \
                    lambda c=ctx[f], rw=rw, rh=rh, W=W, H=H, col=rcol, mot=rmot, out=out, hist=hist, o8=o8, j0=j0, j1=j1: \
                    c.upscale(rw, rh, W, H, col[1], mot[1], out[1], hist[1], mot[0], out[0], hist[0], rgba8_out=o8,
                              jitter_cur=j1, jitter_prev=j0, stream=s)
            ratios.append(dict(render=[rw, rh], display=[W, H], floor_bytes=32 * rw * rh + (20 + 24) * W * H))
        c0.set_camera(cbs[1])
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

    timing = {k: stat(v) for k, v in ms.items()}
    def pass_row(sz, key, **more):
        floor_ms = sz["floor_bytes"] / (COPY_TBS * 1e12) * 1e3
        row = dict(more, render=sz["render"], display=sz["display"], floor_bytes=sz["floor_bytes"], floor_ms=floor_ms)
        for f in FORMS:
            row[f] = dict(timing[key(f)], over_floor=timing[key(f)]["ms"] / floor_ms)
        row["lds_over_direct"] = row["lds"]["ms"] / row["direct"]["ms"]
        lo, hi = sorted(FORMS, key=lambda f: row[f]["ms"])
        row["winner"] = lo if row[lo]["p90"] < row[hi]["p10"] else None  # beyond the spread, or nobody
        return row

    passes = [pass_row(sz, lambda f, H=sz["display"][1]: f"upscale_{f}_{H}", planes_from=name)
              for name, sz in sizes.items()]
    other = [pass_row(sz, lambda f, sz=sz: "upscale_%s_%dx%d_to_%dx%d" % (f, *sz["render"], *sz["display"]),
                      planes_from="C2") for sz in ratios]
    routes = []
    for name, sz in sizes.items():
        r, nat = timing[f"route_{name}"], timing[f"native_{name}"]
        routes.append({"config": name, "render": sz["render"], "display": sz["display"], "spp": sz["spp"], "route": r,
                       "native": nat, "route_over_native": r["ms"] / nat["ms"],
                       "beyond_spread": bool(r["p90"] < nat["p10"] or nat["p90"] < r["p10"])})
    row = {"rounds": a.launches, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "copy_rate_TBps": COPY_TBS,
           "native_library": "a build of the parent commit (--yardstick)" if a.yardstick
           else "this build (no --yardstick given)",
           "passes": passes, "other_ratios": other, "routes": routes, "timing": timing}
    for c in keep:
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
    print(json.dumps({"timing": row}))


if __name__ == "__main__":
    main()
