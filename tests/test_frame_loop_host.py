"""The replay driver of tests/frame_loop_reference.py, pinned without a GPU, so that the reference of
tests/test_gpu_frame_loop.py is checkable on any machine.

The screen-space half runs 6 frames at 37 x 21 (74 x 42 display) over the oracle's G-buffer and motion planes of C2F
under a camera that orbits one manipulator step per frame with Halton jitter, and seeded synthetic raw AO, visibility
and radiance planes: once with the rt.host_* twins, once with the numpy restatements. Tolerance 0: every plane of every
frame equal bit for bit. The input conditions that make the GPU comparison worth something are asserted on the
replay's own output, and one deliberate driver mistake (history from frame k - 2) shows that the comparison can fail.

Measured (printed by the tests): see the assertions' messages; the figures are in DESIGN §3.21.
"""
import ast
import inspect
import os
import re

import numpy as np

import realtimeraytracing_gradproject_amd as rt
from realtimeraytracing_gradproject_amd import scenes

import frame_loop_reference as fl
import materials_reference as mref
import radiance_reference as rref
import reflection_motion_reference as rmref
from frame_loop_reference import bits

W, H, DW, DH, FRAMES = 37, 21, 74, 42, 6
F = np.float32
# C2F's two instances: a rough white teapot that reflects a little, a mirror-like floor
MATERIALS = [mref.MATERIALS[0][:5] + (0.25,), mref.MATERIALS[3][:5] + (0.75,)]
IMAP = np.array([0, 1], np.uint32)
# The three cases in which a 20 % share of changed pixels cannot be reached, each for a reason of the scene, not of the
# replay (measured shares in brackets); they must still change somewhere, and are compared like every other plane:
#   object            an instance index and a hit group: a camera move changes them on silhouettes only (2 - 4 %)
#   normal            C2F's floor is flat, so its normal has the same bits under every camera; only the teapot's pixels
#                     can change (9 - 11 %)
#   hist_up, 1 vs 0   frame 0 has no history (count 1 everywhere) and after the first orbit step the upscaler accepts
#                     history at 4 % of the display pixels only, so the count is 1 again at the other 96 %
# Every other plane, the history counts and the reflection-motion class included, is held to 20 % at every frame pair.
STEADY = {("object", k) for k in range(1, FRAMES)} | {("normal", k) for k in range(1, FRAMES)} | {("hist_up", 1)}

_CACHE = {}


def noise_planes(k, hits, n):
    """Seeded raw planes of frame k in denoise_reference / radiance_reference.synthetic's style, on the surface
    pixels: AO and visibility in {0, 1} (what S = 1 gives), radiance a smooth colour with noise and fireflies and a
    distance in .w; a primary miss holds what the passes write there (1, 1, four zeros)."""
    rng = np.random.default_rng(7000 + k)
    hit = hits[:, 3] == 1
    py, px = np.divmod(np.arange(n), W)
    u = px / W

    def rad():
        base = np.stack([0.2 + 0.5 * u, 0.6 - 0.3 * u, 0.3 + 0.1 * py / H], axis=1)
        rgb = np.abs(base + (0.002 + 0.4 * u ** 2)[:, None] * rng.uniform(-1, 1, (n, 3)))
        fire = rng.random(n) < 0.10
        rgb[fire] *= rng.uniform(3, 30, (int(fire.sum()), 1))
        out = np.concatenate([rgb, rng.uniform(0.5, 20.0, (n, 1))], axis=1).astype(F)
        out[~hit] = 0.0
        return out

    ao = np.where(hit & (rng.random(n) < 0.3), F(0.0), F(1.0)).astype(F)
    vis = np.where(hit & (rng.random(n) < 0.4), F(0.0), F(1.0)).astype(F)[None, :]
    return dict(ao_raw=ao, vis_raw=np.ascontiguousarray(vis), refl=rad(), ind=rad())


def script_and_raw():
    """The script (C2F, orbit + jitter, a static scene) and its raw planes: the oracle's G-buffer and motion, and
    the synthetic planes. Computed once, shared, not modified."""
    if "raw" not in _CACHE:
        base = scenes.config("C2F").with_size(W, H)
        cbs, js = fl.jittered(fl.orbit_cameras(base, FRAMES), W, H)
        frames = [fl.frame_spec(base, cb) for cb in cbs]
        script = fl.Script(W, H, DW, DH, frames, js, list(range(FRAMES)), MATERIALS, IMAP)
        raw = []
        for k, spec in enumerate(frames):
            hits, uv, normal, obj = fl.gbuffer(spec, fl.OracleTracers(spec))
            r = dict(hits=hits, normal=normal, object=obj, motion=fl.motion_plane(spec, frames[max(k - 1, 0)], hits, uv))
            r.update(noise_planes(k, hits, W * H))
            raw.append(r)
        _CACHE["raw"] = (script, raw)
    return _CACHE["raw"]


def replayed(ops=fl.HOST, lag=1):
    key = (ops.name, lag)
    if key not in _CACHE:
        script, raw = script_and_raw()
        _CACHE[key] = fl.replay(script, raw, ops, history_lag=lag)
    return _CACHE[key]


def test_twins_and_numpy_restatements_give_the_same_planes():
    a, b = replayed(fl.HOST), replayed(fl.NUMPY)
    assert a.keys() == b.keys() and len(a) == FRAMES * 29
    for key in sorted(a):
        x, y = bits(a[key]), bits(b[key])
        assert x.shape == y.shape, key
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"frame {key[0]} plane {key[1]}: {bad.shape[0]} of {x.size} words differ, first {bad[0]}"


def test_history_reaches_the_cap_and_stays():
    out = replayed()
    surface = [out[(k, "guide")][:, 3] != 0 for k in range(FRAMES)]
    for plane, col in (("hist", None), ("rmom", 2), ("imom", 2)):
        h = [out[(k, plane)] if col is None else out[(k, plane)][:, col] for k in range(FRAMES)]
        assert all((x[s] <= 4).all() for x, s in zip(h, surface)), f"{plane} exceeds max_history"
        capped = [int(((x == 4) & s).sum()) for x, s in zip(h, surface)]
        print(f"{plane}: surface pixels at history 4 per frame {capped}")
        assert capped[:3] == [0, 0, 0] and capped[3] >= 1 and all(c > 50 for c in capped[4:]), (plane, capped)
    stays = (out[(3, "hist")] == 4) & (out[(4, "hist")] == 4) & (out[(5, "hist")] == 4)
    assert stays.sum() >= 1, "no pixel stays capped over frames 3..5"
    up = [int((out[(k, "hist_up")] == 4).sum()) for k in range(FRAMES)]
    print(f"hist_up: display pixels at history 4 per frame {up}")
    assert all((out[(k, "hist_up")] <= 4).all() for k in range(FRAMES)) and up[3] >= 1 and up[5] > 50


def test_accumulation_classes_and_both_variance_branches():
    out = replayed()
    both = 0
    for k in range(1, FRAMES):
        _, _, cls = rref.accumulate(W, H, out[(k, "refl")], out[(k, "rmotion")], out[(k, "guide")],
                                    out[(k - 1, "racc")], out[(k - 1, "rmom")], out[(k - 1, "guide")], max_history=4)
        counts = {name: int(v.sum()) for name, v in cls.items()}
        surface = ~cls["no_surface"]
        hist = out[(k, "rmom")][:, 2]
        short, full = int((surface & (hist < 4)).sum()), int((surface & (hist >= 4)).sum())
        assert counts["spatial"] == short
        print(f"frame {k}: reflection accumulate {counts}; hist < 4: {short}, hist >= 4: {full}")
        if k >= FRAMES - 3:
            assert counts["blended"] > 50 and counts["disocclusion"] > 20, (k, counts)
        both += short > 0 and full > 0
    assert both >= 1, "no frame has both variance branches"


def test_reflection_motion_reasons():
    out = replayed()
    seen = set()
    for k in range(FRAMES):
        c = rmref.counts(out[(k, "rclass")])
        print(f"frame {k}: reflection motion {c}")
        seen |= {name for name, v in c.items() if v}
    assert "virtual" in seen and len(seen) >= 3, seen


def test_successive_frames_differ():
    out = replayed()
    planes = sorted({p for (_, p) in out})
    for k in range(1, FRAMES):
        s = (out[(k, "guide")][:, 3] != 0) & (out[(k - 1, "guide")][:, 3] != 0)
        shares = {}
        for p in planes:
            a, b = bits(out[(k, p)]), bits(out[(k - 1, p)])
            if p in ("out", "hist_up", "rgba8"):  # display size: every pixel counts
                d = (a != b).reshape(DW * DH, -1).any(axis=1)
                shares[p] = float(d.mean())
            elif a.ndim == 2 and a.shape[0] != W * H:  # per-light planes (L, n)
                shares[p] = float((a != b).any(axis=0)[s].mean())
            else:
                shares[p] = float((a != b).reshape(W * H, -1).any(axis=1)[s].mean())
        print(f"frame {k} vs {k - 1}: " + ", ".join(f"{p} {v:.2f}" for p, v in shares.items()))
        low = {p: v for p, v in shares.items() if v < (0.20 if (p, k) not in STEADY else 1e-9)}
        assert not low, f"frame {k}: planes that change at too few of the pixels: {low}"


def test_a_stale_history_buffer_shows():
    """The driver's one deliberate mistake: every history plane from frame k - 2. The final display frame differs from
    the correct replay at more than a tenth of its pixels, so the GPU comparison fails for that class of bug."""
    good, stale = replayed(), replayed(lag=2)
    last = FRAMES - 1
    differ = (bits(good[(last, "out")]) != bits(stale[(last, "out")])).any(axis=1)
    print(f"history from k - 2: {differ.mean():.3f} of the final frame's pixels differ")
    assert differ.mean() > 0.10
    for p in ("hits", "normal", "object", "motion", "guide"):  # what has no history is the same
        assert np.array_equal(bits(good[(last, p)]), bits(stale[(last, p)]))


def test_the_readme_loop_is_valid_for_the_binding():
    """The README's "whole frame loop" parses, and every ctx.method(...) call in it names a Context method, passes
    no more positional arguments than it takes and only keywords it has; rt.* calls likewise. (The GPU test runs the
    same lines.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "README.md"), encoding="utf-8") as f:
        text = f.read()
    block = re.search(r"The whole frame loop:\n\n```python\n(.*?)```", text, re.S)
    assert block, "the README no longer prints the whole frame loop"
    tree = ast.parse(block.group(1))
    calls = [c for c in ast.walk(tree) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute)
             and isinstance(c.func.value, ast.Name) and c.func.value.id in ("ctx", "rt")]
    names = {c.func.attr for c in calls if c.func.value.id == "ctx"}
    assert {"dispatch_gbuffer_motion", "dispatch_shadow", "denoise_guide", "ao_accumulate", "ao_atrous", "dispatch_ao",
            "dispatch_reflection_chain", "reflection_motion", "radiance_accumulate", "radiance_atrous",
            "dispatch_indirect", "shade_resolve_gi", "upscale", "set_camera"} <= names, names
    for c in calls:
        owner = rt.Context if c.func.value.id == "ctx" else rt
        fn = getattr(owner, c.func.attr, None)
        assert callable(fn), f"README: {c.func.value.id}.{c.func.attr} does not exist"
        params = inspect.signature(fn).parameters
        takes = [p for p in params.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD) and p.name != "self"]
        npos = sum(not isinstance(a, ast.Starred) for a in c.args)
        assert npos <= len(takes), f"README: {c.func.attr} takes {len(takes)} positional arguments, {npos} given"
        for kw in c.keywords:
            assert kw.arg is None or kw.arg in params, f"README: {c.func.attr} has no argument {kw.arg}"
