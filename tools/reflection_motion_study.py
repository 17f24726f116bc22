#!/usr/bin/env python3
"""What the reflection motion plane costs and what it buys: rt_reflection_motion and
rt_radiance_accumulate_reflection from the library's own planes.

static_tol: the largest |e_s - m| (the static point's entry from P = O + D t against the motion plane's, from the
  object vertices through the instance transform) over the surface pixels of C2F at 1920 x 1080 and REFLO at 1280 x 720
  under the tests' camera move (eye + (0.3, 0.15, -0.2)), read off the pass itself: with share = 0 a class-0 entry's
  (mx, my) is e_s bit for bit, and static_tol = 1 px lets every static pixel through (the count of class 3 is reported).

Timing, C2F at 1920 x 1080, in one process, in interleaved rounds (every case once per round), HIP events around each
case on a stream of its own, a sample being 8 launches of the case back to back divided by 8 (one launch is a few tens
of microseconds, too short for one event pair), the order of the cases reversed every other round (a case is faster
right after one that read the same planes), medians with p10 / p90 over the rounds after a warm-up:
  copy                a device-to-device copy of eight 4-float planes' worth of bytes: the copy rate the byte floor is
                      taken at, measured in the same rounds
  motion              rt_reflection_motion alone (guide_prev given, no class plane); floor 68 B per pixel (three 16-byte
                      entries and the distance read, one entry written; the history taps are not in the floor)
  motion_class        the same with class_out
  accumulate          rt_radiance_accumulate alone through the surface motion plane
  two_launches        rt_reflection_motion, then rt_radiance_accumulate through its plane
  fused               rt_radiance_accumulate_reflection
The fused form is kept only if its median lies below two_launches' by more than both p10 - p90 spreads. Every case
writes output planes of its own; after the rounds the two launches and the fused one run once more onto poisoned planes
and their outputs are compared word for word (fused_equals_two_launches).

Quality, C2F at 1920 x 1080 and REFLO at 1280 x 720: 16 frames of a camera orbit about the look-at point (1 degree per
frame), one reflection ray per pixel, accumulated through the surface motion plane and through the reflection motion
plane (each with its own history), then three a-trous iterations on the last frame; RGB RMSE against the same frame's
S = 64 plane, over the pixels with a surface and separately over the flat reflector (the plane hit group) where it
reflects geometry and where it reflects the sky, and over the curved reflectors (the model hit group); at roughness 0
(share 1) and 0.3 (share 1, 0.75, 0.5). The class counts are the last frame's.

  python tools/reflection_motion_study.py --launches 100 --out profiles/reflection_motion_study.json
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import realtimeraytracing_gradproject_amd as rt  # noqa: E402
from realtimeraytracing_gradproject_amd import scenes  # noqa: E402

MOVE = (0.3, 0.15, -0.2)
W, H = 1920, 1080
MOTION_BYTES, COPY_BYTES = 68, 8 * 32
REPS = 8  # launches per timed sample
CLASSES = ("virtual", "no_surface", "no_distance", "moved", "behind", "no_crossing", "no_history")
SCENES = (("C2F", 1920, 1080), ("REFLO", 1280, 720))


def f4(n, dt=torch.float32):
    return torch.zeros((n, 4), dtype=dt, device="cuda")


def f1(n):
    return torch.zeros((n,), dtype=torch.float32, device="cuda")


def with_eye(spec, eye):
    s = scenes.SceneSpec(**{**spec.__dict__})
    s.camera = (tuple(float(v) for v in eye), spec.camera[1], spec.camera[2])
    return s


def orbit(spec, deg):
    eye, center, _ = spec.camera
    a = math.radians(deg)
    dx, dz = eye[0] - center[0], eye[2] - center[2]
    return with_eye(spec, (center[0] + dx * math.cos(a) + dz * math.sin(a), eye[1],
                           center[2] - dx * math.sin(a) + dz * math.cos(a)))


def context(spec):
    c = rt.Context(0)
    c.set_motion_history(True)
    scenes.upload(c, spec)
    return c


def counts(cls):
    b = torch.bincount(cls.long(), minlength=7).cpu().tolist()
    return dict(zip(CLASSES, b))


def static_distance(name, w, h, ts):
    spec = scenes.config(name).with_size(w, h)
    prev = with_eye(spec, [a + b for a, b in zip(spec.camera[0], MOVE)])
    n, s = w * h, ts.cuda_stream
    c = context(spec)
    hits, normal, motion, guide, rad, out = f4(n, torch.int32), f4(n), f4(n), f4(n), f4(n), f4(n)
    cls = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    c.dispatch_gbuffer_motion(w, h, hits=hits, normal=normal, motion=motion, prev_camera=prev.camera_buffer(), stream=s)
    c.denoise_guide(n, normal, motion.view(-1)[3:], guide, stream=s)
    c.reflection_motion(w, h, hits, guide, motion, rad.view(-1)[3:], spec.camera_buffer(), prev.camera_buffer(), out,
                        class_out=cls, share=0.0, static_tol=1.0, stream=s)
    ts.synchronize()
    v = cls == 0
    d = (out[v, :2].double() - motion[v, :2].double()).abs()
    r = {"width": w, "height": h, "eye_move": MOVE, "classes": counts(cls),
         "largest_abs_es_minus_m_px": float(d.max()), "p99_px": float(torch.quantile(d.max(dim=1).values[::7], 0.99))}
    c.forget_stream(s)
    c.close()
    return r


def quality(name, w, h, ts, frames=16, step_deg=1.0):
    base = scenes.config(name).with_size(w, h)
    n, s = w * h, ts.cuda_stream
    c = context(orbit(base, 0.0))
    hits, normal, motion, rad, truth = f4(n, torch.int32), f4(n), f4(n), f4(n), f4(n)
    obj = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    guides = [f4(n), f4(n)]
    cls = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    vm, flt, var, tmp, vtmp = f4(n), f4(n), f1(n), f4(n), f1(n)
    cases = [("roughness_0", 0.0, 1.0), ("roughness_0.3_share_1", 0.3, 1.0), ("roughness_0.3_share_0.75", 0.3, 0.75),
             ("roughness_0.3_share_0.5", 0.3, 0.5)]
    out = {"width": w, "height": h, "frames": frames, "orbit_deg_per_frame": step_deg, "reference": "S = 64, seed 1000"}
    for label, rough, share in cases:
        hist = {r: [(f4(n), f4(n)), (f4(n), f4(n))] for r in ("surface", "virtual")}
        for k in range(frames):
            cur, prev = orbit(base, k * step_deg), orbit(base, max(k - 1, 0) * step_deg)
            cb, pcb = cur.camera_buffer(), prev.camera_buffer()
            g, gp = guides[k % 2], guides[(k - 1) % 2]
            c.set_camera(cb)
            c.dispatch_gbuffer_motion(w, h, hits=hits, normal=normal, object=obj, motion=motion, prev_camera=pcb,
                                      stream=s)
            c.denoise_guide(n, normal, motion.view(-1)[3:], g, stream=s)
            c.dispatch_reflection(w, h, rad, 1, rough, seed=k, stream=s)
            if k:
                c.reflection_motion(w, h, hits, g, motion, rad.view(-1)[3:], cb, pcb, vm, guide_prev=gp, class_out=cls,
                                    share=share, stream=s)
            for route, plane in (("surface", motion), ("virtual", vm)):
                o, p = hist[route][k % 2], hist[route][(k - 1) % 2]
                if k == 0:
                    c.radiance_accumulate(w, h, rad, motion, g, o[0], o[1], stream=s)
                else:
                    c.radiance_accumulate(w, h, rad, plane, g, o[0], o[1], p[0], p[1], gp, stream=s)
        c.dispatch_reflection(w, h, truth, 64, rough, seed=1000, stream=s)
        last, g = (frames - 1) % 2, guides[(frames - 1) % 2]
        ts.synchronize()
        surface = g[:, 3] != 0
        t64 = truth.double()[:, :3]
        # where: every surface pixel; the flat reflector (the plane hit group) where the S = 64 rays mostly hit geometry
        # (mean distance below half of tmax) and where they mostly missed; the curved reflectors (the model hit group)
        flat = surface & (obj[:, 1] == rt.RT_HITGROUP_PLANE)
        near = truth[:, 3] < 500.0
        groups = {"all": surface, "flat_reflecting_geometry": flat & near, "flat_reflecting_sky": flat & ~near,
                  "curved": surface & ~flat}

        def rmse(x, sel):
            return float(torch.sqrt(torch.mean((x.double()[:, :3][sel] - t64[sel]) ** 2)))

        row = {"roughness": rough, "share": share, "pixels": {k: int(v.sum()) for k, v in groups.items()},
               "classes": counts(cls), "classes_flat": counts(cls[flat]), "classes_curved": counts(cls[groups["curved"]]),
               "rmse_S1_raw": {k: rmse(rad, v) for k, v in groups.items()}}
        for route in ("surface", "virtual"):
            acc, mom = hist[route][last]
            c.radiance_atrous(w, h, acc, mom, g, flt, var, tmp, vtmp, iterations=3, stream=s)
            ts.synchronize()
            for tag, x in (("accumulated", acc), ("filtered", flt)):
                row[f"rmse_{route}_{tag}"] = {k: rmse(x, v) for k, v in groups.items()}
            row[f"mean_history_{route}"] = {k: float(mom[:, 2][v].mean()) for k, v in groups.items()}
        row["virtual_over_surface_filtered"] = {k: row["rmse_virtual_filtered"][k] / row["rmse_surface_filtered"][k]
                                                for k in groups}
        out[label] = row
    c.forget_stream(s)
    c.close()
    return out


def timing(ts, launches, warmup):
    spec = scenes.config("C2F").with_size(W, H)
    prev = with_eye(spec, [a + b for a, b in zip(spec.camera[0], MOVE)])
    cb, pcb = spec.camera_buffer(), prev.camera_buffer()
    n, s = W * H, ts.cuda_stream
    c = context(prev)
    hits, normal, motion, guide, gprev, rad = f4(n, torch.int32), f4(n), f4(n), f4(n), f4(n), f4(n)
    prev_rad, prev_mom, vm, acc, mom = f4(n), f4(n), f4(n), f4(n), f4(n)
    acc2, mom2, acc_s, mom_s = f4(n), f4(n), f4(n), f4(n)  # every case writes planes of its own
    cls = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    copy_src, copy_dst = f4(8 * n), f4(8 * n)
    c.dispatch_gbuffer_motion(W, H, hits=hits, normal=normal, motion=motion, stream=s)
    c.denoise_guide(n, normal, motion.view(-1)[3:], gprev, stream=s)
    c.dispatch_reflection(W, H, rad, 1, 0.0, seed=0, stream=s)
    c.radiance_accumulate(W, H, rad, motion, gprev, prev_rad, prev_mom, stream=s)
    c.set_camera(cb)
    c.dispatch_gbuffer_motion(W, H, hits=hits, normal=normal, motion=motion, prev_camera=pcb, stream=s)
    c.denoise_guide(n, normal, motion.view(-1)[3:], guide, stream=s)
    c.dispatch_reflection(W, H, rad, 1, 0.0, seed=1, stream=s)
    ts.synchronize()
    dist = rad.view(-1)[3:]

    def copy():
        with torch.cuda.stream(ts):
            copy_dst.copy_(copy_src)

    def two():
        c.reflection_motion(W, H, hits, guide, motion, dist, cb, pcb, vm, guide_prev=gprev, stream=s)
        c.radiance_accumulate(W, H, rad, vm, guide, acc, mom, prev_rad, prev_mom, gprev, stream=s)

    runs = {
        "copy": copy,
        "motion": lambda: c.reflection_motion(W, H, hits, guide, motion, dist, cb, pcb, vm, guide_prev=gprev, stream=s),
        "motion_class": lambda: c.reflection_motion(W, H, hits, guide, motion, dist, cb, pcb, vm, guide_prev=gprev,
                                                    class_out=cls, stream=s),
        "accumulate": lambda: c.radiance_accumulate(W, H, rad, motion, guide, acc_s, mom_s, prev_rad, prev_mom, gprev,
                                                    stream=s),
        "two_launches": two,
        "fused": lambda: c.radiance_accumulate_reflection(W, H, rad, motion, guide, hits, cb, pcb, acc2, mom2, prev_rad,
                                                          prev_mom, gprev, stream=s),
    }
    ms = {k: [] for k in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    order = list(runs.items())
    for k in range(warmup + launches):
        # odd rounds run the cases in reverse: a case follows another that left its inputs in the last-level cache, and
        # this way each of two neighbours is the follower half of the time
        for name, fn in (order if k % 2 == 0 else order[::-1]):
            e0.record(ts)
            for _ in range(REPS):  # a sample is REPS launches back to back: one launch is a few tens of microseconds
                fn()
            e1.record(ts)
            ts.synchronize()
            if k >= warmup:
                ms[name].append(e0.elapsed_time(e1) / REPS)
    # the contract at this size, on launches of its own: poisoned outputs, the two launches, the fused one, word for word
    for t_ in (vm, acc, mom, acc2, mom2):
        t_.view(torch.int32).fill_(0x2B2B2B2B)
    torch.cuda.synchronize()
    two()
    runs["fused"]()
    ts.synchronize()
    a1, a2, m1, m2 = (t_.view(torch.int32) for t_ in (acc, acc2, mom, mom2))
    same = bool(torch.equal(a1, a2) and torch.equal(m1, m2))
    differing_words = int((a1 != a2).sum() + (m1 != m2).sum())
    copy_ms = float(np.median(ms["copy"]))
    copy_tbs = n * COPY_BYTES / (copy_ms * 1e-3) / 1e12
    floor_ms = n * MOTION_BYTES / (copy_tbs * 1e12) * 1e3

    def stat(v):
        v = np.asarray(v, np.float64)
        return {"ms": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}

    t = {k: stat(v) for k, v in ms.items()}
    for k in ("motion", "motion_class"):
        t[k]["over_floor"] = t[k]["ms"] / floor_ms
    two_, fu = t["two_launches"], t["fused"]
    spreads = (two_["p90"] - two_["p10"]) + (fu["p90"] - fu["p10"])
    row = {"config": "C2F", "width": W, "height": H, "rounds": launches, "warmup": warmup, "eye_move": MOVE,
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "copy_rate_TBps": copy_tbs, "motion_floor_bytes_per_pixel": MOTION_BYTES, "motion_floor_ms": floor_ms,
           "classes": counts(cls), "timing": t, "fused_equals_two_launches": same, "fused_differing_words": differing_words,
           "launches_per_sample": REPS,
           "fused_over_two_launches": fu["ms"] / two_["ms"], "fused_saving_ms": two_["ms"] - fu["ms"],
           "sum_of_both_spreads_ms": spreads, "fused_earns_its_place": bool(two_["ms"] - fu["ms"] > spreads)}
    c.forget_stream(s)
    c.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.launches < 100:
        sys.exit("reflection_motion_study: at least 100 timed rounds")
    if not torch.cuda.is_available():
        sys.exit("reflection_motion_study: needs the GPU (nothing is measured without one)")
    ts = torch.cuda.Stream()
    doc = {"static_tol": {name: static_distance(name, w, h, ts) for name, w, h in SCENES}}
    worst = max(v["largest_abs_es_minus_m_px"] for v in doc["static_tol"].values())
    doc["static_tol"]["largest_px"] = worst
    doc["static_tol"]["default"] = min(0.25, 2.0 ** math.ceil(math.log2(16.0 * worst))) if worst > 0 else 0.0
    doc["static_tol"]["binding_default"] = rt.REFLECTION_MOTION_STATIC_TOL
    doc["timing"] = timing(ts, a.launches, a.warmup)
    doc["quality"] = {name: quality(name, w, h, ts) for name, w, h in SCENES}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
