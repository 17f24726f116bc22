#!/usr/bin/env python3
"""Per-frame cost of animating one mesh: rt_blas_rebuild + full rt_tlas_build against rt_blas_refit(_device) +
rt_tlas_build(update_only = 1), and what keeping the old topology costs a frame (DESIGN: BLAS refit).

For the teapot and the rabbit (the largest mesh of scenes.py), each with the ground plane:
  rebuild      rt_blas_rebuild (host vertices) + rt_tlas_build(update_only = 0)
  refit_device rt_blas_refit_device (a device tensor) + rt_tlas_build(update_only = 1)
  refit_host   rt_blas_refit (host vertices) + rt_tlas_build(update_only = 1)
one context per path, the paths taken in turn inside every step (one process, interleaved), a new smooth deformation
of the mesh per step. Host wall: a clock around the two calls (both return after their kernels have completed).
Device time: build_ms of rt_blas_info + rt_tlas_info (the calls' own events). Medians over the steps after a warm-up.
Frames: the mesh's 1080p LAMBERT_SHADOW config (C2 / C3) on the refitted tree after a 10 % deformation against a
context that built the deformed mesh from scratch, device events around each dispatch, interleaved, medians.

  python tools/refit_study.py --steps 60 --out profiles/refit_study.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import realtimeraytracing_gradproject_amd as rt  # noqa: E402
from realtimeraytracing_gradproject_amd import scenes  # noqa: E402


def deform(verts, amount, seed=3):
    """A smooth displacement of `amount` x the mesh extent (a function of the position: shared vertices stay shared)."""
    v = np.array(verts, dtype=np.float32, copy=True)
    rng = np.random.default_rng(seed)
    p = v[:, :3].astype(np.float64)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    freq = rng.uniform(1.0, 3.0, size=(3, 3)) * (2.0 * np.pi / ext)
    phase = rng.uniform(0.0, 2.0 * np.pi, size=3)
    v[:, :3] = (p + amount * ext * np.sin(p @ freq.T + phase)).astype(np.float32)
    return v


def med(x):
    return float(np.median(np.asarray(x, np.float64)))


def study(config, steps, warmup, frames):
    spec = scenes.config(config)
    verts, idx = spec.meshes[0]
    paths = ("rebuild", "refit_device", "refit_host")
    ctx = {p: rt.Context(0) for p in paths}
    ids = {p: scenes.upload(ctx[p], spec) for p in paths}
    inst = {p: [(ids[p][m], x, iid, hg) for (m, x, iid, hg) in spec.instances] for p in paths}
    wall = {p: [] for p in paths}
    dev = {p: [] for p in paths}
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(warmup + steps):
        dv = deform(verts, 0.1 * np.sin(0.37 * (k + 1)))
        d_dv = torch.from_numpy(dv).cuda()
        torch.cuda.synchronize()
        for p in paths:
            c, b = ctx[p], ids[p][0]
            t0 = time.perf_counter()
            if p == "rebuild":
                c.blas_rebuild(b, dv, idx)
                c.tlas_build(inst[p])
            elif p == "refit_device":
                c.blas_refit_device(b, d_dv, stream=stream)
                c.tlas_build(inst[p], update_only=True)
            else:
                c.blas_refit(b, dv)
                c.tlas_build(inst[p], update_only=True)
            t1 = time.perf_counter()
            if k >= warmup:
                wall[p].append((t1 - t0) * 1e3)
                dev[p].append(c.blas_info(b).build_ms + c.tlas_info().build_ms)
    row = {"config": config, "model": spec.model, "triangles": int(idx.size // 3), "vertices": int(verts.shape[0]),
           "steps": steps, "warmup": warmup}
    info = ctx["refit_device"].blas_info(ids["refit_device"][0])
    row["nodes"], row["depth"] = int(info.node_count), int(info.depth)
    for p in paths:
        row[f"{p}_wall_ms"] = med(wall[p])
        row[f"{p}_wall_ms_min"] = float(np.min(wall[p]))
        row[f"{p}_device_ms"] = med(dev[p])
    row["refit_beats_rebuild_wall"] = bool(row["refit_device_wall_ms"] < row["rebuild_wall_ms"])
    # frame time on the refitted tree against a fresh build of the same deformed mesh
    dv = deform(verts, 0.1)
    ctx["refit_device"].blas_refit_device(ids["refit_device"][0], torch.from_numpy(dv).cuda(), stream=stream)
    ctx["refit_device"].tlas_build(inst["refit_device"], update_only=True)
    ctx["rebuild"].blas_rebuild(ids["rebuild"][0], dv, idx)
    ctx["rebuild"].tlas_build(inst["rebuild"])
    out = torch.zeros((spec.height, spec.width, 4), dtype=torch.uint8, device="cuda")
    ms = {"refit_device": [], "rebuild": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pics = {}
    ts = torch.cuda.Stream()  # a stream of its own: a null stream handle would mean the context's stream
    for k in range(10 + frames):
        for p in ms:
            e0.record(ts)
            ctx[p].dispatch(spec.width, spec.height, out, stream=ts.cuda_stream)
            e1.record(ts)
            torch.cuda.synchronize()
            if k >= 10:
                ms[p].append(e0.elapsed_time(e1))
            pics[p] = out.cpu().numpy() if k == 0 else pics[p]
    row["frame_ms_refitted_tree"] = med(ms["refit_device"])
    row["frame_ms_fresh_tree"] = med(ms["rebuild"])
    row["frames_equal"] = bool(np.array_equal(pics["refit_device"], pics["rebuild"]))
    for c in ctx.values():
        c.forget_stream(ts.cuda_stream)
        c.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default=os.path.join("profiles", "refit_study.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("refit_study: needs the GPU (nothing is measured without one)")
    rows = [study(cfg, a.steps, a.warmup, a.frames) for cfg in ("C2", "C3")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
